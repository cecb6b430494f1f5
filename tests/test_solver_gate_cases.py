"""The solver gate cases of tests/solver_gate_cases.py without a device: their literal launch rows against the CPU build of the
device's own classification (oracle/csrc/mf_host.cpp: mf_analyze with the device's options, then classify_launches), that both
sides of the gates are reached, and that the exact backward-error check of tests/test_gpu_solver_gates.py cannot hide a lost
term."""
import numpy as np
import pytest

import solver_gate_cases as S

ETA_MAX = S.ETA_MAX         # asserted equal to tests/test_gpu_solver.py's in tests/test_gpu_solver_gates.py
NAMES = [c.name for c in S.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_literal_rows_are_the_rows_of_the_cpu_classification(name):
    from collections import Counter
    c = S.CASE[name]
    rows, fronts = S.host_rows(name, with_fronts=True)
    assert rows == c.rows
    # the fronts themselves (level, m, k, children, how many): the rows carry only max_m / max_k of a launch
    assert tuple(k + (v,) for k, v in sorted(Counter(map(tuple, fronts.tolist())).items())) == c.fronts
    for env, rows in c.switched.items():
        assert S.host_rows(name, env) == rows, env
        if env != S.OLD_BIG or any(r["inv"] for r in c.rows):
            assert rows != c.rows, (env, "the switch changes nothing here")


def _some(pred, env=None):
    return [(c.name, r) for c in S.CASES for r in (c.switched.get(env, ()) if env else c.rows) if pred(r)]


def test_both_sides_of_every_gate_are_reached():
    lds = lambda r: r["cls"] and not r["tiny"]
    for cls, lo in ((16, None), (32, 17), (48, 33), (64, 49), (88, 65), (128, 89)):        # each class at m = c, the next at c + 1
        assert _some(lambda r: r["cls"] == cls and r["max_m"] == cls and r["count"] > 0), cls
        assert lo is None or _some(lambda r: lds(r) and r["cls"] == cls and r["max_m"] == lo), cls
    assert [f for f in S.CASE["m16"].fronts if f[:3] == (0, 16, 3)] and [f for f in S.CASE["m16"].fronts if f[:3] == (1, 16, 15)]
    assert [f for f in S.CASE["m17"].fronts if f[:3] == (0, 17, 3)] and [f for f in S.CASE["m33"].fronts if f[:3] == (0, 33, 3)]
    assert S.CASE["m16"].rows[0]["tiny"] and not S.CASE["m17"].rows[0]["tiny"] and not S.CASE["m16"].rows[1]["tiny"]
    # packed leaves: every parent an LDS front (packed) against a parent on the large-front path (square), by the plan alone
    for name, packed, parent_cls, asm in (("leaf_lds", True, 128, "none"), ("leaf_big_inv", False, 0, "columns"),
                                          ("leaf_big_subst", False, 0, "gather")):
        r = S.CASE[name].rows
        assert r[0]["tiny"] and r[0]["packed"] == packed and (r[2]["cls"], r[2]["assembly"]) == (parent_cls, asm), name
    assert S.CASE["leaf_big_inv"].rows[0]["max_m"] == 16 and S.CASE["leaf_big_inv"].rows[2]["inv"]
    # k = 1 on the large-front path in both generations, and folded by merge rule 1; k = 64 / 65 with m = 129
    assert (0, 202, 1, 0, 1) in S.CASE["k1_subst"].fronts and not S.CASE["k1_subst"].rows[0]["inv"] and S.CASE["k1_subst"].rows[0]["cls"] == 0
    assert S.CASE["k1_subst"].switched[S.INV_ALWAYS][0]["inv"]
    assert (0, 132, 1, 0, 1) in S.CASE["k1_inv"].fronts and S.CASE["k1_inv"].rows[0]["inv"] and S.CASE["k1_inv"].rows[0]["count"] == 12
    assert not S.CASE["k1_inv"].switched[S.OLD_BIG][0]["inv"]
    c = S.CASE["k1_rule1"]
    assert (0, 66, 1, 0, 1) in c.fronts and (0, 129, 64, 0, 1) in c.fronts and (0, 129, 31, 0, 1) in c.fronts
    assert (c.rows[0]["cls"], c.rows[0]["count"], c.rows[0]["inv"]) == (0, 12, True)
    # merge rule 1 accepted: the LDS-sized fronts inside the large-front launch, with m - k = 63, 64, 65
    f = {x[:3] for x in S.CASE["rule1_accept"].fronts}
    assert {(0, 76, 11), (0, 94, 31), (0, 95, 32), (0, 97, 33), (0, 103, 40), (0, 129, 65), (0, 129, 66), (0, 129, 100)} <= f
    assert _some(lambda r: r["cls"] == 128 and r["max_m"] == 128) and _some(lambda r: r["cls"] == 0 and r["max_m"] == 129)
    assert _some(lambda r: r["tiny"] and r["packed"]) and _some(lambda r: r["tiny"] and not r["packed"], S.NO_PACKED)
    assert _some(lambda r: r["cls"] == 16 and not r["tiny"] and r["level"] > 0)                 # m <= 16 above level 0
    assert _some(lambda r: r["wave"] and r["cls"] == 48 and r["max_child"] == 0) and _some(lambda r: r["wave"] and r["cls"] == 16)
    assert _some(lambda r: not r["wave"] and r["cls"] == 48, S.NO_WAVE)
    # inverse-based path: n = 1023 against 1024 with the same large fronts
    a, b = S.CASE["n1023"].rows[0], S.CASE["n1024"].rows[0]
    assert (a["max_m"], a["max_k"], a["count"]) == (b["max_m"], b["max_k"], b["count"]) and not a["inv"] and b["inv"]
    # assembly: childless and 9+ children column-tiled, 1 and 7 children gathered; block 0 of all three kinds, 23 against 24 fronts
    assert _some(lambda r: r["assembly"] == "columns" and r["max_child"] == 0) and _some(lambda r: r["assembly"] == "columns" and r["max_child"] > 8)
    assert _some(lambda r: r["assembly"] == "gather" and r["max_child"] == 1) and _some(lambda r: r["assembly"] == "gather" and r["max_child"] == 7)
    assert _some(lambda r: r["block0"] == "gather") and _some(lambda r: r["block0"] == "diag0" and r["count"] == 24)
    assert _some(lambda r: r["block0"] == "step0" and r["count"] == 23)
    assert _some(lambda r: r["cls"] == 0 and not r["inv"], S.OLD_BIG)
    # merge rule 2: a merged launch with mixed m and k, and the same fronts unmerged
    assert len(S.CASE["merged_mixed"].rows) < len(S.CASE["merged_mixed"].switched[S.NO_MERGE])
    # merge rule 2 at count 255 / 256 (4 count >= next.count on both sides: 255 / 256 decides)
    a, b = S.CASE["merge255"].rows, S.CASE["merge256"].rows
    assert a[0]["count"] == 256 and a[0]["cls"] == 88 and (b[0]["count"], b[0]["cls"], b[1]["count"], b[1]["cls"]) == (256, 64, 1, 88)
    # merge rule 1: accepted at lds_count = big count (8 LDS-sized fronts, m 76 ... 103, k 11 ... 40, inside the large-front launch
    # of 16 with k up to 100), refused at big count + 1, and refused by a group with m <= 32 alone (7 <= 8 fronts)
    a, b, c = S.CASE["rule1_accept"].rows[0], S.CASE["rule1_count"].rows, S.CASE["rule1_m32"].rows
    assert (a["cls"], a["count"], a["inv"]) == (0, 16, True) and sum(r["count"] for r in S.CASE["rule1_accept"].switched[S.NO_MERGE] if r["level"] == 0 and r["cls"]) == 8
    assert (b[0]["cls"], b[0]["count"], b[1]["cls"], b[1]["count"]) == (128, 9, 0, 8)
    assert (c[0]["cls"], c[0]["count"], c[1]["cls"], c[1]["count"]) == (128, 7, 0, 8)
    # large-front assembly at 8 / 9 children and at max_child max_m = 10 240 / 10 241
    assert S.CASE["ch8"].rows[1]["max_child"] == 8 and S.CASE["ch8"].rows[1]["assembly"] == "gather"
    assert S.CASE["ch9"].rows[1]["max_child"] == 9 and S.CASE["ch9"].rows[1]["assembly"] == "columns"
    a, b = S.CASE["edge10240"].rows[2], S.CASE["edge10241"].rows[2]
    assert a["max_child"] * a["max_m"] == 10240 and a["assembly"] == "gather" and b["max_child"] * b["max_m"] == 10241 and b["assembly"] == "columns"
    # wave: a child with m - k = 8 against 9; LDS sweeps at max_k = 8 / 9 / 16 / 17; 16 / 17 children of an LDS front
    assert S.CASE["wave_c8"].rows[2]["wave"] and S.CASE["wave_c8"].rows[2]["max_child"] == 1 and not S.CASE["wave_c9"].rows[2]["wave"]
    for name, k, variant in (("k8", 8, "k8"), ("k9", 9, "k16"), ("k16", 16, "k16"), ("k17", 17, "general")):
        assert (S.CASE[name].rows[0]["max_k"], S.CASE[name].rows[0]["backward"]) == (k, variant), name
    assert S.CASE["ch16"].rows[1]["max_child"] == 16 and S.CASE["ch17"].rows[1]["max_child"] == 17
    assert all(r["cls"] for name in ("ch16", "ch17") for r in S.CASE[name].rows)


def test_fast_exact_residual_is_the_rational_one():
    for name, grade in (("tiny", 12), ("lds64", 0), ("lds64", 12), ("big129", 12)):
        A, g, _ = S.system(name, grade)
        x = S.reference(name, grade) * (1.0 + 2.0 ** -30)
        assert np.array_equal(S.exact_residual(A, x, g), S.exact_residual_rational(A, x, g)), (name, grade)


@pytest.mark.parametrize("tag", [z[0] for z in S.ZERO_PIVOTS])
def test_zero_pivot_matrices_have_their_zero_pivot_where_they_say(tag):
    """An un-pivoted dense LDL' in the plan's elimination order meets its first zero pivot exactly at the chosen unknown."""
    A, g, x_ref, j = S.zero_pivot_system(tag)
    name = S.ZERO[tag][1]
    b = S.built(name)
    _, _, order = S.host_launches(*S.pattern(name), S.centroids(S.N_ELEMENTS, b.elements, b.m), with_order=True)
    perm = order[:b.m]
    M = A.toarray()[np.ix_(perm, perm)]
    stop = int(np.flatnonzero(perm == j)[0])
    for c in range(stop + 1):
        d = M[c, c]
        if c == stop:
            assert d == 0.0, (tag, d)
            break
        assert d != 0.0
        l = M[c + 1:, c] / d
        M[c + 1:, c + 1:] -= np.outer(l, M[c + 1:, c])
    assert np.linalg.norm(A @ x_ref - g) <= 1e-10 * np.linalg.norm(g)


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_exact_and_the_bound_cannot_hide_a_lost_term(name):
    """x_ref has eta <= 2^-50; dropping or doubling any single entry of A, or perturbing any single x_j by 2^-20 relative, pushes
    eta above 64 ETA_MAX -- for 100 % of 512 seeded samples per (case, grade).  The mutations are applied to the exact residual
    and the denominators of the affected row; an x_j perturbation is judged in row j alone (its diagonal term), which is a
    lower bound of what the whole column would show."""
    for grade in S.CASE[name].grades:
        A, g, _ = S.system(name, grade)
        x = S.reference(name, grade)
        r = S.exact_residual(A, x, g)
        den = S.denominators(A, x, g)
        assert np.max(np.abs(r) / den) <= 2.0 ** -50, (name, grade)
        rng = np.random.default_rng(7 + grade)
        rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
        pick = rng.choice(A.nnz, min(512, A.nnz), replace=False)
        i, j, a = rows[pick], A.indices[pick], A.data[pick]
        term = a * x[j]
        for delta, dden in ((-term, -np.abs(term)), (term, np.abs(term))):            # the entry dropped / doubled
            e = np.abs(r[i] + delta) / (den[i] + dden)
            assert np.all(e > 64 * ETA_MAX), (name, grade, float(e.min()))
        jj = rng.choice(A.shape[0], min(512, A.shape[0]), replace=False)             # x_j (1 + 2^-20): seen in row j
        dx = x[jj] * 2.0 ** -20
        ajj = A.diagonal()[jj]
        e = np.abs(r[jj] + ajj * dx) / (den[jj] + np.abs(ajj * dx))
        assert np.all(e > 64 * ETA_MAX), (name, grade, float(e.min()))
