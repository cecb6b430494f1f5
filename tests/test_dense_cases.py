"""The dense-path cases of tests/dense_cases.py without a device: the claimed tile / block / ring shapes against the kernel
arithmetic, the references against the oracle's own fp64 closures, the sensitivity condition with its never-skipped rows and
columns, and NumPy restatements of the kernels' sums with one term dropped or doubled, which the bounds must reject (a check
that cannot fail checks nothing)."""
import math

import numpy as np
import pytest

import dense_cases as D
from gate_cases import KERNEL_RTOL, MAX_SKIPPED, SENSITIVITY


def _id(v):
    return v if isinstance(v, str) else str(v)


def test_claimed_shapes_hold():
    for case in D.CASES:
        assert D.check_claims(case)
    f = {c.name: D.shape_facts(c, c.sizes[0]) for c in D.CASES}
    # the literals once more, independent of the claims table: csrc/dense.hip's constants are GT = 64, GK = 16, unroll 3
    assert (f["n65"]["nkt_plan"], f["n65"]["nkt_H"]) == (5, 9) and f["n65"]["gemv_empty_waves"] == (13, 14, 15)
    assert (f["n96"]["nkt_plan"] % 3, f["n96"]["nkt_H"] % 3) == (0, 0) and f["n96"]["nkt_H"] == 12
    assert {f[k]["nkt_H"] % 3 for k in f} == {0, 1, 2}
    assert f["n256"]["node_blocks"] == 1 and f["n257"]["node_blocks"] == 2 and f["n257"]["last_node_block"] == 1
    assert f["n257"]["gemv_t_tail"] == 1 and f["n257_wide"]["active_rows"] == 6
    first_op = {c.name: {a: nm for a, nm in reversed(c.D_spec)} for c in D.CASES}     # per state: the operator of its first D row
    assert [k for k, v in first_op.items() if v[0] != "id"] == ["n65_dx_first"]       # the one case that starts with gemv_t<false>
    sizes = {m for c in D.CASES if c.n > 64 for m in c.sizes[:-1]}
    assert {63, 64, 65, 128, 129} <= sizes
    assert D.CASE["n64"].coarse == D.CASE["n65"].coarse[1:]          # both sides of the p > 64 gate see the same levels
    b = D.built("n257_masked")
    assert np.all(b.bw[list(D.MASKED_NODES)] == 0) and np.count_nonzero(b.bw) == 257 - 5 and not np.any(b.bw == 1.0)


@pytest.mark.parametrize("name", [c.name for c in D.CASES])
def test_problem_is_rounded_bounded_away_from_zero_and_inside_the_cone(name):
    b = D.built(name)
    for nm, op in b.ops.items():
        assert np.array_equal(op * D.ONE, np.rint(op * D.ONE))
        if nm == "id":
            assert b.M.geometry.operators[nm].is_identity()
        else:
            assert 0.29 <= np.abs(op).min() and np.abs(op).max() <= 1.0 and (op < 0).any() and (op > 0).any()
            assert not b.M.geometry.operators[nm].is_identity()
    n = b.case.n
    assert np.array_equal(b.z0[-n:], np.rint(b.z0[-n:]))
    for level in range(len(b.R)):
        o = D.oracle_node(name, level)
        assert np.all(np.isfinite(o["F"])) and np.all(o["slack"] < 0)
        Dz = o["Dz"]
        q = np.sqrt(sum(Dz[:, k] ** 2 for k in b.case.idx[:-1]))
        assert np.all(Dz[:, b.case.idx[-1]] >= 3.9 * q ** D.P_CONE)                  # well inside the cone
        f0, f0_abs = D.f0_reference(name, level)
        assert f0_abs <= 4.0 * abs(f0)


@pytest.mark.parametrize("name,level", D.LEVELS, ids=_id)
def test_references_agree_with_the_oracle_and_meet_the_sensitivity_condition(name, level):
    from oracle import mgb_oracle as O
    b = D.built(name)
    z, dz = D.dz_reference(name, level)
    Mo = O.OracleAMG(b.M)
    s, c, z0 = D.inputs(name, level)
    assert np.array_equal(z, z0 + b.R[level] @ s)                                    # exact in fp64, in any order
    Dz_o = O.apply_D(Mo.D_fine, z)
    assert np.all(np.abs(Dz_o - dz.value) <= dz.bound)
    y_o, g_o, H_o = D.oracle_closures(name, level)
    f0, _ = D.f0_reference(name, level)
    assert abs(y_o - f0) <= KERNEL_RTOL * abs(f0)
    f1, f2 = D.f1_reference(name, level), D.f2_reference(name, level)
    assert f1.ratios(g_o).max() <= 1.0 and np.all(np.abs(g_o - f1.value) <= f1.bound)
    assert f2.ratios(H_o).max() <= 1.0 and np.all(np.abs(H_o - f2.value) <= f2.bound)
    for ref in (dz, f1, f2):
        assert ref.skipped <= MAX_SKIPPED, (name, level, ref.skipped)
        assert np.all(ref.sensitive[ref.never & (ref.abssum > 0)]), (name, level)
    assert np.all(f1.abssum > 0) and np.all(dz.abssum > 0)
    m = b.R[level].shape[1]
    if level + 1 < len(b.R):
        assert np.all(f2.abssum > 0)
        edges = sorted({i % m for i in D.NEVER_SKIPPED if -m <= i < m})
        assert f2.never[edges, :].all() and f2.never[:, edges].all()


def _violates(ref, shape, index, value):
    """A device result equal to the reference except at `index`: the check the device tests assert on must reject it."""
    dev = ref.value.copy().reshape(shape)
    dev[index] = value
    return ref.ratios(dev).max() > 1.0


F2_ENTRIES = [("n257", 0, 0, 64), ("n257", 0, 64, 0), ("n257", 0, 64, 64), ("n257", 0, 63, 64), ("n257", 0, 0, 0), ("n257", 0, 31, 40),
              ("n257", 1, 0, 128), ("n257", 1, 128, 0), ("n257", 1, 64, 128), ("n257", 1, 128, 128), ("n65", 3, 0, 64), ("n65", 3, 64, 0),
              ("n96", 0, 64, 64), ("n129", 1, 128, 63)]


@pytest.mark.parametrize("name,level,i,j", F2_ENTRIES, ids=_id)
def test_f2_without_or_with_twice_a_term_violates_the_bound(name, level, i, j):
    """H_ij restated as the H GEMM sums it (K index = active row x node, K tiles of 16): without the last node's term, without
    the whole last K tile, without the smallest term, with the first term twice; and the mirrored store left out."""
    ref = D.f2_reference(name, level)
    n = D.CASE[name].n
    kidx, vals = D.f2_terms(name, level, i, j)
    nz = np.flatnonzero(vals)
    assert abs(math.fsum(vals.tolist()) - ref.value[i, j]) <= ref.bound[i, j]
    K = kidx.max() + 1
    last_tile = nz[kidx[nz] >= D.GK * ((K - 1) // D.GK)]
    last_node = nz[kidx[nz] % n == n - 1]
    smallest = nz[np.argmin(np.abs(vals[nz]))]
    assert last_node.size > 0
    muts = [("last node", -vals[last_node[0]]), ("smallest", -vals[smallest]), ("first twice", vals[nz[0]])]
    if last_tile.size:                 # the last K tile belongs to the slack's id row: rows i of H in the slack columns reach it
        muts.append(("last K tile", -math.fsum(vals[last_tile].tolist())))
    else:
        assert i < D.built(name).cols[level][-1][0]
    for what, delta in muts:
        assert abs(delta) >= SENSITIVITY * ref.bound[i, j], (what, abs(delta) / ref.bound[i, j])
        assert _violates(ref, ref.value.shape, (i, j), ref.value[i, j] + delta), what
    if i // D.GT != j // D.GT:         # the symmetric variant stores C[col + ldc * row] = val: a missing mirror leaves a zero
        assert abs(ref.value[i, j]) >= SENSITIVITY * ref.bound[i, j] and _violates(ref, ref.value.shape, (i, j), 0.0)


@pytest.mark.parametrize("level,j", [(0, 0), (0, 31), (1, 0), (1, 63), (2, 0), (2, 256)])
def test_f1_without_the_last_node_violates_the_bound(level, j):
    """g_j restated as gemv_t sums it (ret_a = sum over rows = nodes, lanes striding by 64: node 256 is the one row of the
    fifth stride), without node 256 and with it twice."""
    name = "n257"
    b = D.built(name)
    n = b.case.n
    ref = D.f1_reference(name, level)
    Y = D.oracle_node(name, level)["Y"]
    assert b.cols[level][0][0] <= j < b.cols[level][0][1]
    Ru = b.R[level][:n, j]
    ret = Y[:, 0] + b.D[1].T @ Y[:, 1]
    assert abs(Ru @ ret - ref.value[j]) <= ref.bound[j]
    delta = Ru @ (b.D[1][n - 1, :] * Y[n - 1, 1])
    one = np.abs(Ru * b.D[1][n - 1, :] * Y[n - 1, 1])
    assert one[one > 0].min() >= SENSITIVITY * ref.bound[j]                           # a single product of that row already
    for d in (-delta, delta):
        assert abs(d) >= SENSITIVITY * ref.bound[j]
        assert _violates(ref, ref.value.shape, (j,), ref.value[j] + d)


def test_f0_and_Dz_without_the_last_node_violate_their_bounds():
    name = "n257"
    for level in range(len(D.built(name).R)):
        f0, _ = D.f0_reference(name, level)
        t = D.oracle_node(name, level)["f0_terms"]
        assert t.size == 257
        # the second out_partial is node 256 alone: lost or counted twice
        assert abs(t[256]) >= SENSITIVITY * KERNEL_RTOL * abs(f0)
        assert abs(math.fsum(t[:256].tolist()) - f0) > KERNEL_RTOL * abs(f0)
        z, dz = D.dz_reference(name, level)
        dx = D.built(name).D[1]
        last = np.abs(dx[:, 256] * z[256])                                            # the last column's term of every row of dx z
        assert np.all(last >= SENSITIVITY * dz.bound[:, 1])
        assert _violates(dz, dz.value.shape, (256, 1), 0.0) and _violates(dz, dz.value.shape, (64, 1), dz.value[64, 1] - last[64])
        assert _violates(dz, dz.value.shape, (256, 0), 0.0)


def test_extended_and_exact_sums_agree(monkeypatch):
    """The rational fall-back of platforms without an 80-bit long double gives the same references (smallest level)."""
    refs = {}
    for ext in (D.EXTENDED, False):
        monkeypatch.setattr(D, "EXTENDED", ext)
        monkeypatch.setattr(D, "UREF", 2.0 ** -64 if ext else 0.0)
        D.f1_reference.cache_clear(); D.f2_reference.cache_clear()
        refs[ext] = (D.f1_reference("n65", 0), D.f2_reference("n65", 0))
    D.f1_reference.cache_clear(); D.f2_reference.cache_clear()
    for a, b in zip(refs[D.EXTENDED], refs[False]):
        assert np.all(np.abs(a.value - b.value) <= 2.0 ** -52 * np.abs(b.value))
        assert np.all(np.abs(a.value - b.value) <= a.bound)
