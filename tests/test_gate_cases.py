"""The gate cases of tests/gate_cases.py without a device: the expected plans against a restatement of the gate arithmetic,
the exact references against the oracle's own fp64 products, the sensitivity condition, and mutated references that the bound
must reject (a check that cannot fail checks nothing)."""
from fractions import Fraction

import numpy as np
import pytest

import gate_cases as G

LEVELS = [(c.name, l) for c in G.CASES for l in range(len(c.all_levels()))]
REFS = ([("prolong", *q) for q in G.op_params("prolong")] + [("restrict", *q) for q in G.op_params("restrict")] +
        [("assemble", *q) for q in G.op_params("assemble")])
BUILD = {"prolong": G.prolong_reference, "restrict": G.restrict_reference, "assemble": G.assemble_reference}


def _id(v):
    return v if isinstance(v, str) else str(v)


def test_exact_sum_is_the_fraction_sum():
    rng = np.random.default_rng(3)
    a, b, c = (rng.standard_normal(200) * 10.0 ** rng.uniform(-8, 8, 200) for _ in range(3))
    assert G.exact_sum(a, b) == sum(Fraction(x) * Fraction(y) for x, y in zip(a, b))
    assert G.exact_sum(a, b, c) == sum(Fraction(x) * Fraction(y) * Fraction(z) for x, y, z in zip(a, b, c))
    assert G.exact_sum(np.zeros(0), np.zeros(0)) == 0


@pytest.mark.parametrize("name,level", LEVELS, ids=_id)
def test_expected_plan_is_what_the_gate_arithmetic_gives(name, level):
    case = G.CASE[name]
    lv = case.all_levels()[level]
    plan = G.restated_plan(G.level_R(name, level), case.N)
    for key, want in lv.expect.items():
        assert plan[key] == want, (name, lv.name, key, plan[key], want)
    if lv.ops:
        assert np.isfinite(G.oracle_f0(name, level)), "the evaluation point must lie inside the cone"
    for env, projection in lv.switches:
        assert G.restated_plan(G.level_R(name, level), case.N, no_mfma=env == "MGBHIP_NO_MFMA_PROJECT")["projection"] == projection


def test_every_variant_is_expected_on_both_sides_of_its_gate():
    """The literals of gate_cases.CASES cover the table of DESIGN.md ("Shape gates")."""
    exp = [lv.expect for c in G.CASES for lv in c.all_levels() if lv.ops]
    asm = [lv.expect for c in G.CASES for lv in c.all_levels() if "assemble" in lv.ops]
    for key in ("R_unit", "R_long", "T_long"):
        assert {e[key] for e in exp} == {True, False}, key
    assert {0, 1, 2, 3, 33} <= {e["T_chunks"] for e in exp}
    assert {e["max_col"] for e in exp} >= {64, 65, 1023, 1024, 4096, 4097, 8193} and {e["max_row"] for e in exp} >= {1, 64, 65}
    assert {e["acc"] for e in asm} == {True, False} and {e["long_lists"] for e in asm} == {True, False}
    assert {e["selection"] for e in asm} == {True, False}
    assert {e["gather_nchunk"] for e in asm} == {0, 64}
    proj = {e["projection"] for e in asm} | {p for c in G.CASES for lv in c.all_levels() for _, p in lv.switches}
    assert proj == {"none", "loop", "staged", "mfma", "accumulate"}
    assert {49, 48} <= {e.get("mean_list") for e in asm}


def test_two_stage_gather_lists_sit_on_the_chunk_edges():
    lens = G.list_lengths(G.level_R("gather_two_stage", 0), G.CASE["gather_two_stage"].N).diagonal()
    chunk = G.CASE["gather_two_stage"].levels[0].expect["gather_chunk"]
    assert sorted(lens.tolist()) == [16 * chunk - 1, 16 * chunk, 16 * chunk + 1, 64 * chunk]


@pytest.mark.parametrize("op,name,level", REFS, ids=_id)
def test_reference_is_sensitive_and_agrees_with_the_oracle(op, name, level):
    ref = BUILD[op](name, level)
    live = ref.abssum > 0
    # the sensitivity condition: the smallest non-zero term of a checked entry is >= 64 bounds; <= 5 % may miss it
    skipped = 1.0 - float(ref.sensitive[live].mean())
    assert skipped <= G.MAX_SKIPPED, (op, name, level, skipped)
    # the oracle's own fp64 product against the exact one, within the rounding term of the bound alone
    if op == "restrict":
        o = G.oracle_f1(name, level)[ref.index]
    elif op == "assemble":
        o = G.dense_H(G.oracle_f2(name, level), G.level_R(name, level).shape[1])[ref.index]
    else:
        s, _, z0 = G.inputs(name, level)
        o = (z0 + G.level_R(name, level) @ s)[ref.index]
    assert np.all(np.abs(o - ref.value) <= ref.length * G.U53 * ref.abssum), (op, name, level)


@pytest.mark.parametrize("op,name,level", REFS, ids=_id)
def test_a_dropped_or_doubled_term_violates_the_bound(op, name, level):
    """On the longest, the shortest and eight seeded entries: the reference without its smallest term, and with the first term
    of every chunk (CHUNK entries of a restriction row, gather_chunk summands of a list) doubled, is off by >= 64 bounds in
    exact arithmetic, and `Reference.ratios` -- the check the device tests assert on -- reports a violation."""
    ref = BUILD[op](name, level)
    use = np.flatnonzero(ref.sensitive & (ref.abssum > 0))
    nterm = np.array([len(ref.terms[k][0]) for k in use])
    rng = np.random.default_rng(5)
    picks = {int(use[np.argmax(nterm)]), int(use[np.argmin(nterm)]), *rng.choice(use, min(8, use.size), replace=False).tolist()}
    step = G.CASE[name].all_levels()[level].expect.get("gather_chunk") or G.CHUNK
    dev = np.zeros(int(ref.index.max()) + 1)
    for k in picks:
        fs = ref.terms[k]
        prod = np.abs(np.prod(np.stack(fs), axis=0))
        drop = int(np.argmin(np.where(prod > 0, prod, np.inf)))
        muts = [ref.exact[k] - G.exact_sum(*[f[drop:drop + 1] for f in fs])]
        for t in range(0, len(fs[0]), step):
            if prod[t] > 0:
                muts.append(ref.exact[k] + G.exact_sum(*[f[t:t + 1] for f in fs]))
        for mut in muts:
            assert abs(mut - ref.exact[k]) >= G.SENSITIVITY * Fraction(float(ref.bound[k])), (op, name, level, k)
            dev[ref.index] = ref.value
            dev[ref.index[k]] = float(mut)
            assert ref.ratios(dev).max() > 1.0, (op, name, level, k)


def test_reduction_inputs_have_exact_products():
    B = G.reduce_block_cap()
    assert B == 1024 and G.reduction_lengths()[-1] > 256 * B + 256
    a, b = G.reduction_vectors(257)
    assert all(Fraction(x) * Fraction(y) == Fraction(x * y) for x, y in zip(a.tolist(), b.tolist()))
    assert np.abs(a).max() / np.abs(a).min() > 1e10 and (a < 0).any() and (a > 0).any()


def test_solve_hierarchy_has_a_chunked_and_a_row_parallel_level():
    prob = G.solve_problem()
    for R, expect in zip(prob.M[0].R_fine, G.SOLVE_PLANS, strict=True):
        plan = G.restated_plan(G.sp.csr_matrix(R), 2048)
        assert {k: plan[k] for k in expect} == expect
