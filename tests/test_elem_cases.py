"""The element-kernel cases of tests/elem_cases.py without a device: the claimed plans against the restated gate arithmetic,
the sensitivity condition with its never-skipped entries, deliberate errors in the reference computation which the bounds must
reject by a factor SENSITIVITY (a check that cannot fail checks nothing), the oracle's closed cone formulas against 50-digit
derivatives of the barrier's definition, and the extended host check of csrc/elem_layout.hpp."""
import numpy as np
import pytest

import elem_cases as E
from gate_cases import KERNEL_RTOL, MAX_SKIPPED, SENSITIVITY

NAMES = [c.name for c in E.CASES]


def _id(v):
    return v if isinstance(v, str) else str(v)


def test_claimed_plans_hold():
    for case in E.CASES:
        assert E.check_claims(case)
    kinds = {(E.restated_plan(c, "f2")["kind"], E.restated_plan(c, "f2")["NY"], E.restated_plan(c, "f2")["P"]) for c in E.CASES}
    # every entry of the fast table with a runtime signature, the five default ones a hand-built D table can have, every
    # generic NY the table names, the wide kernel
    for ny, p in E.FAST_TABLE:
        assert ("fast_runtime", ny, p) in kinds or ("fast_default", ny, p) in kinds, (ny, p)
    for want in [("fast_default", 3, 2), ("fast_default", 4, 7), ("fast_default", 5, 8), ("fast_default", 4, 6), ("fast_default", 7, 7),
                 ("fast_runtime", 3, 2), ("fast_runtime", 4, 7), ("fast_runtime", 6, 2), ("fast_runtime", 7, 7), ("fast_runtime", 8, 8),
                 ("fast_runtime", 7, 6), ("wide", 0, 0)] + [("generic", ny, 0) for ny in (1, 2, 3, 4, 8, 9, 10)]:
        assert want in kinds, want
    other = {E.restated_plan(c, "f0")["NY"] for c in E.CASES if E.restated_plan(c, "f0")["kind"] == "generic"}
    assert set(range(1, 11)) == other                                    # generic<1> .. generic<10> in the non-f2 modes
    # workgroup edges: N = EPB + 1, N = EPB and N = 1 for a fast and a generic variant each
    for mode in ("f2", "f0"):
        by = {(c.N - E.restated_plan(c, mode)["EPB"]) for c in E.CASES if c.name.startswith("p2_default") and not c.phase1}
        assert {1, 0} <= by and 1 in {c.N for c in E.CASES}
    assert E.restated_plan(E.CASE["p7_default_n32"], "f2")["grid"] == 1 and E.restated_plan(E.CASE["p7_default"], "f2")["grid"] == 2
    w = E.CASE["wide_nd7"]
    assert (E.restated_plan(w, "f2")["threads"], E.restated_plan(w, "f01")["threads"]) == (128, 256)
    assert E.restated_plan(E.CASE["p32_tile_edge"], "f2")["nstage"] * (256 // 32) * 32 * 32 * 8 == 64 * 1024     # exactly 64 KiB
    assert (E.restated_plan(E.CASE["p33_mixed"], "f2")["nstage"], E.restated_plan(E.CASE["p33_mixed"], "f2")["unstaged"]) == (1, 1)


@pytest.mark.parametrize("name", NAMES)
def test_problem_is_rounded_and_inside_the_cone(name):
    b = E.built(name)
    case = b.case
    for (a, nm), Dk in zip(case.D_full, b.D):
        assert np.array_equal(Dk * E.ONE, np.rint(Dk * E.ONE))
        if nm == "id":
            assert b.M.geometry.operators[nm].is_identity()
        else:
            assert 0.29 <= np.abs(Dk).min() and np.abs(Dk).max() <= 1.0
            assert case.N == 1 or not np.array_equal(Dk[0], Dk[-1])          # every element has its own block
            assert not b.M.geometry.operators[nm].is_identity()
    sel = b.sel.reshape(case.nu, case.n)
    for a in range(case.nu):
        empty = sel[a] < 0
        assert empty.any() == (a not in case.slack_states and case.n > 2), (name, a)       # both branches of zsel >= 0
    assert np.array_equal(np.sort(b.sel[b.sel >= 0]), np.arange(b.R[1].shape[1]))          # one row per column
    assert sorted(set(np.diff(b.R[0].indptr))) != [0, 1]                                   # level 0 is not a selection level
    inside = np.ones(case.n, dtype=bool)
    inside[b.outside] = False
    for level in (0, 1):
        for pt in ("base", "trial"):
            ev = E.element_eval(name, level, pt)
            assert np.all(np.isfinite(ev["F"][inside])), (name, level, pt)
            if case.masked:
                assert not np.any(np.isfinite(ev["F"][b.outside]))          # outside the cone: -log of a negative number
                assert np.all(b.bw[b.outside] == 0)
            if ev["slack"] is not None:
                assert np.all(ev["slack"][inside] < 0)
            f0, f0_abs = E.f0_reference(name, level, pt)
            assert np.isfinite(f0) and f0_abs <= 4.0 * abs(f0)
    if case.masked:
        assert len(b.outside) * 2 == len(E.masked_nodes(case)) and np.count_nonzero(b.bw == 0) == len(E.masked_nodes(case))


@pytest.mark.parametrize("name,level", E.LEVELS, ids=_id)
def test_references_meet_the_sensitivity_condition(name, level):
    for pt in ("base", "trial"):
        for ref in (E.f1_reference(name, level, pt), E.f2_reference(name, level, pt)):
            assert np.all(np.isfinite(ref.value))
            assert ref.skipped <= MAX_SKIPPED, (name, level, pt, ref.skipped)
            live = ref.abssum > 0
            assert not np.any(ref.never & live & ~ref.sensitive), (name, level, pt)
            assert np.all(ref.value[~live] == 0.0)
    if level == 1:
        H = E.f2_reference(name, level)
        assert np.all(np.abs(H.value - H.value.T) <= H.bound)        # A' H A of the oracle is symmetric up to its own rounding


def test_references_agree_with_the_oracles_own_closures():
    """The references are built from the oracle's per-node g and H; its f0 / f1 / f2 closures (sparse products in fp64) must
    agree with them within the references' own bounds."""
    import scipy.sparse as sp
    from oracle import mgb_oracle as O
    for name in ("p2_default", "p7_general_cone", "ny9", "wide_nd7_phase1", "p6_masked"):
        b = E.built(name)
        Mo = O.OracleAMG(b.M)
        B = O.Barrier(b.Qo, b.bw)
        for level in (0, 1):
            s, c, z0 = E.inputs(name, level)
            args = (s, Mo.w, c, Mo.R_fine[level], Mo.D_fine, z0)
            f0, _ = E.f0_reference(name, level)
            with np.errstate(all="ignore"):
                assert abs(B.f0(*args) - f0) <= KERNEL_RTOL * abs(f0)
                assert E.f1_reference(name, level).ratios(B.f1(*args)).max() <= 1.0
                H = np.asarray(sp.csr_matrix(B.f2(*args)).todense())
            assert E.f2_reference(name, level).ratios(np.nan_to_num(H) if b.case.masked else H).max() <= 1.0


def _violation(ref, mutated):
    use = ref.sensitive & (ref.abssum > 0)
    d = np.abs(mutated.value[use] - ref.value[use]) / ref.bound[use]
    d = np.where(np.isfinite(mutated.value[use]), d, np.inf)
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("mut", E.MUTATIONS)
def test_a_deliberate_error_breaks_the_bound(mut):
    """element e with element e - 1's operator block or z, node p - 1 dropped, two Y rows swapped, one term dropped or doubled,
    a masked node not masked: each must violate the bound by >= SENSITIVITY on a checked entry of every case with the feature."""
    hit = 0
    for case in E.CASES:
        if not E.applies(case, mut):
            continue
        hit += 1
        worst = max(_violation(ref(case.name, 1), ref(case.name, 1, "base", mut)) for ref in (E.f1_reference, E.f2_reference))
        assert worst >= SENSITIVITY, (case.name, mut, worst)
        if mut in ("op_shift", "z_shift"):          # visible in Dz itself, which the device must return bit for bit
            assert not np.array_equal(E.element_eval(case.name, 1)["Dz"], E.element_eval(case.name, 1, "base", mut)["Dz"])
    assert hit >= 1


# ---- the common mode of oracle and kernel: closed derivative formulas -----------------------------------------------------

def _mp_barrier(b, node):
    """The node barrier F(y) from its definition (mpmath), for the case's Convex or its phase-I wrapper."""
    import mpmath as mp
    case, Q = b.case, b.Q
    NC = case.NC

    def piece(pc, k, y, extra):
        if Q.select is not None and Q.select[node, k] == 0:
            return mp.mpf(0)
        ni = pc.ni
        if pc.kind == E.KIND_EP:
            z = [sum(mp.mpf(float(pc.A[node, r + ni * c])) * y[pc.idx[c]] for c in range(ni)) + mp.mpf(float(pc.b[node, r])) for r in range(ni)]
            s = z[ni - 1] + extra
            p0, mu = mp.mpf(float(pc.p[node])), mp.mpf(float(pc.mu[node]))
            return -mp.log(s ** (2 / p0) - sum(q * q for q in z[:ni - 1])) - mu * mp.log(s)
        nc = pc.nc
        return -sum(mp.log(sum(mp.mpf(float(pc.A[node, r + nc * c])) * y[pc.idx[c]] for c in range(ni)) + mp.mpf(float(pc.b[node, r])) + extra)
                    for r in range(nc))

    def F(*y):
        if not case.phase1:
            return sum(piece(pc, k, y, 0) for k, pc in enumerate(Q.pieces))
        u = y[NC - 1]
        bb, RR = mp.mpf(b.box[0]), mp.mpf(b.box[1])
        out = sum(piece(pc, k, y, u) for k, pc in enumerate(Q.pieces)) - mp.log(bb - u) - mp.log(bb + u)
        return out - sum(mp.log(RR - v) + mp.log(RR + v) for v in y[NC:])
    return F


def sample_nodes(case):
    """Every node of the first and last element of each workgroup, filled up to at least 64 nodes."""
    nodes = np.flatnonzero(E.never_nodes(case).reshape(case.N, case.p).all(axis=1).repeat(case.p))
    rest = np.setdiff1d(np.arange(case.n), nodes)
    more = rest[np.linspace(0, rest.size - 1, max(0, min(64 - nodes.size, rest.size))).astype(int)] if rest.size else rest
    return np.union1d(nodes, more)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_cone_formulas_agree_with_50_digit_derivatives_of_the_definition(name):
    """F from the definition, g and H by mpmath.diff (no closed derivative formula): the oracle's fp64 F, g, H must agree to
    KERNEL_RTOL / SENSITIVITY of the node's largest |g| resp. |H| entry -- a condition on the evaluation points, checked here."""
    mp = pytest.importorskip("mpmath", reason="the 50-digit reference of the node barrier needs mpmath")
    from oracle import mgb_oracle as O
    b = E.built(name)
    case = b.case
    nD = case.nD
    tol = KERNEL_RTOL / SENSITIVITY
    Dz = E.element_eval(name, 1)["Dz"]
    with np.errstate(all="ignore"):
        Fo, Go, Ho = (O.node_eval(b.Qo, Dz, k) for k in (0, 1, 2))
    nodes = np.setdiff1d(sample_nodes(case), b.outside)
    assert nodes.size >= min(64, case.n) - len(b.outside)
    act = [k for k in range(nD) if (E.restated_plan(case, "f2")["ymask"] >> k) & 1]
    for k in range(nD):
        if k not in act:
            assert not Go[:, k].any() and not Ho[:, k, :].any()
    with mp.workdps(50):
        for node in nodes:
            F = _mp_barrier(b, int(node))
            y = tuple(mp.mpf(float(v)) for v in Dz[node])
            assert abs(F(*y) - mp.mpf(float(Fo[node]))) <= tol * max(abs(F(*y)), 1), (name, node)
            gmax, hmax = np.abs(Go[node]).max(), np.abs(Ho[node]).max()
            for i, k in enumerate(act):
                o1 = tuple(1 if j == k else 0 for j in range(nD))
                assert abs(mp.diff(F, y, o1) - mp.mpf(float(Go[node, k]))) <= tol * gmax, (name, node, k)
                for k2 in act[i:]:
                    if not Ho[:, k, k2].any() and node != nodes[0]:
                        continue              # rows of different pieces: a structural zero, differentiated at one node only
                    o2 = tuple((1 if j == k else 0) + (1 if j == k2 else 0) for j in range(nD))
                    assert abs(mp.diff(F, y, o2) - mp.mpf(float(Ho[node, k, k2]))) <= tol * hmax, (name, node, k, k2)
                    assert abs(Ho[node, k, k2] - Ho[node, k2, k]) <= tol * hmax


def test_host_check_of_the_dispatch_decision():
    """tests/csrc/elem_layout_check.cpp (stand-alone, g++, -fsanitize=address,undefined): elem_decide over the whole
    (p, nu, nD, nstage) grid against the launchers' former predicates."""
    from test_elem_layout_host import test_layout_sizes_equal_the_launchers_former_formulas as run
    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        run(pathlib.Path(d))
