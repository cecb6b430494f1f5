"""The cone-wall cases of tests/wall_cases.py without a device: claimed plans, decidable points on the right side of the wall, the
closed formulas of the 50-digit reference against mp.diff of the barrier's definition, the oracle's fp64 formulas within a quarter of
every bound (so the points and the operation count are right before any GPU run), and deliberate errors in the fp64 formulas, each
of which must break a bound by SENSITIVITY -- the near-wall ones at a node with k >= 16 too."""
import mpmath as mp
import numpy as np
import pytest

import elem_cases as E
import wall_cases as W
from gate_cases import SENSITIVITY
from test_elem_cases import _mp_barrier


def test_claimed_plans_and_grid_coverage():
    kinds = set()
    for case in W.CASES:
        assert W.check_claims(case)
        if case.dense:
            kinds.add(("dense", len(case.pieces[0][1]) > E.NARROW_W))
            continue
        for mode in E.MODES:
            r = W.expected_plan(case.name, mode)
            kinds.add((r["kind"], r["NY"], r["P"]))
            assert r["grid"] == 2 or (r["kind"] == "wide" and mode == "f2" and r["grid"] == 3), (case.name, mode, r)     # N = EPB + 1
    for want in [("fast_default", 4, 7), ("fast_default", 3, 2), ("fast_runtime", 7, 7), ("generic", 5, 0), ("generic", 9, 0), ("wide", 0, 0),
                 ("dense", False), ("dense", True)]:
        assert want in kinds, want
    ks, es, ps, nqs = set(), set(), set(), set()
    for case in W.CASES:
        b = W.built(case.name)
        ks |= set(int(k) for k in b.knode["base"])
        for pc in b.Q.pieces:
            if pc.kind == W.EP:
                ps |= set(pc.p.tolist())
                nqs.add(pc.ni - 1)
        s = b.pts["base"][(case.nu0 - 1) * case.n:case.nu0 * case.n]
        es |= set(int(e) for e in np.round(np.log2(s) / 10))
    assert ks >= set(W.GRID_K) and ps == set(W.GRID_P) and nqs >= {1, 2, 3, 4}
    assert {-10, -2, 0, 2, 10} <= es, es                         # magnitudes of s from 2^-100 to 2^100


@pytest.mark.parametrize("name", W.NAMES)
def test_points_are_exact_decidable_and_on_their_side(name):
    """built() asserts, for every point: A y + b and y_s + slack exact, q of <= 20 bits at the tuned nodes, every active piece
    decidable, outside exactly at the nodes the point names.  Here: the trial and outside points are the once-rounded steps."""
    from test_gpu_elem import exact_step
    b = W.built(name)
    case = b.case
    for pt in ("trial", "outside"):
        assert np.array_equal(b.pts[pt], exact_step(b.pts["base"], b.dirs[pt], W.TRIAL_STEP))
        assert np.any(b.pts[pt] != b.pts["base"])
    assert 3 <= len(b.out_nodes) <= 6
    assert set(b.knode["outside"][b.out_nodes]) <= set(W.OUT_K) | set(W.GRID_K) and len(set(b.knode["outside"][b.out_nodes])) >= 2
    for pt in W.POINTS:
        ref = W.reference(name, pt)
        assert np.array_equal(np.flatnonzero(~ref.inside), b.out_nodes if pt == "outside" else [])
        assert np.all(np.isposinf(ref.F[~ref.inside])) and np.all(np.isfinite(ref.F[ref.inside]))
        assert np.isposinf(ref.f0) == (pt == "outside")
        assert np.all(ref.Fb[ref.inside & (ref.F != 0)] > 0) and np.all(ref.f1b[np.tile(ref.inside, case.nu)] > 0)      # (F = 0: every piece deselected)
        assert np.array_equal(ref.f2 != 0, ref.f2b != 0) and np.allclose(ref.f2, ref.f2.T, rtol=1e-15, atol=0)
        assert np.count_nonzero(ref.knode >= W.NEAR_K) >= 20
    if case.phase1:
        Dz = W.dz_at(b, "base")
        bb, RR = b.box
        NC = case.NC
        assert np.min(bb - np.abs(Dz[:, NC - 1])) == bb * 2.0 ** -40 and np.min(RR - np.abs(Dz[:, NC:])) == RR * 2.0 ** -40
        assert np.any(Dz[:, NC - 1] < 0) and np.any(Dz[:, NC] < 0)            # both sides of both boxes


@pytest.mark.parametrize("name", W.NAMES)
def test_closed_formulas_agree_with_derivatives_of_the_definition(name):
    """F from the definition, g and H by mpmath.diff at 80 digits (near the wall the barrier varies on the scale r, far below the
    scale of s): the closed formulas of the reference must agree to 1e-30 of the node's largest entry, on >= 64 nodes."""
    b = W.built(name)
    case = b.case
    nD = case.nD
    Dz = W.dz_at(b, "base")
    nodes = np.unique(np.rint(np.linspace(0, case.n - 1, 72)).astype(int))
    assert nodes.size >= 64
    for node in nodes:
        mp.mp.dps = W.DPS
        nd = W._node(b, int(node), tuple(float(v) for v in Dz[node]))
        act = [k for k in range(nD) if nd["G"][k].t or nd["H"][k][k].t]
        if not act:                  # every piece deselected at this node
            assert nd["F"] == 0 and b.Q.select is not None and not b.Q.select[node].any()
            continue
        with mp.workdps(80):
            F = _mp_barrier(b, int(node))
            y = tuple(mp.mpf(float(v)) for v in Dz[node])
            assert abs(F(*y) - nd["F"]) <= mp.mpf(10) ** -30 * max(abs(nd["F"]), 1), (name, node)
            gmax = max(abs(nd["G"][k].v) for k in act)
            hmax = max(abs(nd["H"][k][k2].v) for k in act for k2 in act)
            for i, k in enumerate(act):
                o1 = tuple(1 if j == k else 0 for j in range(nD))
                assert abs(mp.diff(F, y, o1) - nd["G"][k].v) <= mp.mpf(10) ** -30 * gmax, (name, node, k)
                for k2 in act[i:]:
                    if not nd["H"][k][k2].t and node != nodes[0]:
                        continue
                    o2 = tuple((1 if j == k else 0) + (1 if j == k2 else 0) for j in range(nD))
                    assert abs(mp.diff(F, y, o2) - nd["H"][k][k2].v) <= mp.mpf(10) ** -30 * hmax, (name, node, k, k2)
                    assert abs(nd["H"][k][k2].v - nd["H"][k2][k].v) <= mp.mpf(10) ** -40 * hmax
        for k in range(nD):
            if k not in act:
                assert not any(nd["H"][k][k2].t for k2 in range(nD))


@pytest.mark.parametrize("name", W.NAMES)
def test_the_oracle_stays_within_a_quarter_of_every_bound(name):
    """The fp64 closed formulas with libm at every entry of every point: if this fails, the points or the operation count are wrong."""
    for pt in W.POINTS:
        ref = W.reference(name, pt)
        F, G, H, slack = W.fp64_node_eval(name, pt)
        assert np.all(np.isposinf(F[~ref.inside])), (name, pt)
        f0, f1, f2 = W.assemble_fp64(name, pt, F, G, H)
        assert np.isposinf(f0) == (pt == "outside")
        r = W.ratios(ref, F=F, slack=slack, f0=f0, f1=f1, f2=f2)
        for what, (worst, _) in r.items():
            assert worst <= W.ORACLE_SHARE, (name, pt, what, worst)
    if any(len(idx) > E.NARROW_W for _, idx, _ in W.CASE[name].pieces):
        # the wide path's algebra (projector + rank two), restated in fp64, is the same Hessian
        ref = W.reference(name, "base")
        F, G, H, _ = W.fp64_node_eval(name, "base", "wide_algebra")
        r = W.ratios(ref, f2=W.assemble_fp64(name, "base", F, G, H)[2])
        assert r["f2"][0] <= W.ORACLE_SHARE, (name, r)


@pytest.mark.parametrize("mut", W.MUTATIONS)
def test_a_deliberate_error_breaks_a_bound(mut):
    hit = 0
    for case in W.CASES:
        if not W.applies(case, mut):
            continue
        hit += 1
        ref = W.reference(case.name, "base")
        F, G, H, _ = W.fp64_node_eval(case.name, "base", mut)
        f0, f1, f2 = W.assemble_fp64(case.name, "base", F, G, H)
        r = W.ratios(ref, F=F, f1=f1, f2=f2)
        worst = max(v[0] for v in r.values())
        near = max(v[1] for v in r.values())
        assert worst >= SENSITIVITY, (case.name, mut, r)
        if mut in W.NEAR_WALL:
            assert near >= SENSITIVITY, (case.name, mut, r)
    assert hit >= 1, mut
