"""Every evaluation of the node barrier (csrc/cone.hpp: ep_identity_eval, piece_accumulate, wide_piece, cone_slack) next to the
cone wall on the device (DESIGN.md "Cone wall"): the hand-built problems of tests/wall_cases.py against their 50-digit references,
within bounds that follow the conditioning of r = s^(2/p) - |q|^2 (no 1e-10 floor, no skipped entry).  Each test asserts, in this
order: the plan, Dz bit for bit, F / slack / f0 / f1 / f2 / one line-search trial within their bounds, f2 bitwise symmetric and
bitwise repeatable, and the points outside the cone as +inf / finite == 0.  The worst error / bound per case and path is
recorded (helpers.record_observation); nothing is asserted from the record."""
import numpy as np
import pytest

import elem_cases as E
import wall_cases as W
from helpers import record_observation

pytestmark = pytest.mark.gpu

PLAN_KEYS = ("kind", "NY", "P", "threads", "G", "EPB", "grid", "lds", "nstage", "unstaged", "ymask")
FINEST = 1
_live = {}


def open_case(name):
    from mgb_amd.device import DeviceProblem, HipContext
    b = W.built(name)
    ctx = HipContext(0)
    P = DeviceProblem(ctx, b.M, b.Q, feasibility=b.case.phase1, NC=b.case.NC, barrier_weights=None)
    if b.case.phase1:
        P.set_box(*b.box)
    return ctx, P


def _close_all():
    for ctx, P in _live.values():
        P.close()
        ctx.close()
    _live.clear()


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    _close_all()


def device(name):
    if name not in _live:
        _close_all()                             # one resident problem at a time
        _live[name] = open_case(name)
    return _live[name][1]


def assert_plan(P, name):
    """The kernel each mode runs, before any number."""
    for mode in E.MODES:
        got, want = P.elem_plan(mode), W.expected_plan(name, mode)
        keys = ("kind",) if W.CASE[name].dense else PLAN_KEYS
        assert {k: got[k] for k in keys} == {k: want[k] for k in keys}, (name, mode, got, want)
        assert got["newton_kind"] == got["kind"], (name, mode, got)
    return P.elem_plan("f2")["kind"], P.elem_plan("f1")["kind"]


def _fmt(r):
    return ", ".join(f"{k} {v[0]:.3f}" for k, v in r.items())


@pytest.mark.parametrize("name", W.NAMES)
def test_barrier_at_the_cone_wall(name):
    P = device(name)
    b = W.built(name)
    case = b.case
    n = case.n
    kind_f2, kind_other = assert_plan(P, name)
    c, z0 = b.c, b.z0
    x, xt, xo = (b.pts[pt] for pt in W.POINTS)
    ref, ref_t, ref_o = (W.reference(name, pt) for pt in W.POINTS)
    # Dz, bit for bit
    z = P.prolong_add(FINEST, P.vec(x), P.vec(z0)).to_host()
    assert np.array_equal(z, x), name
    F, Dz = P.node_barrier(z, want_Dz=True)
    assert np.array_equal(Dz, ref.Dz), (name, np.argwhere(Dz != ref.Dz)[:4])
    # the numbers at the base point and one trial
    slack = None if case.phase1 else P.node_slack(z)
    y = P.f0(FINEST, x, c, z0)
    g = P.f1(FINEST, x, c, z0)
    H = np.asarray(P.f2(FINEST, x, c, z0).todense())
    assert H.shape == ref.f2.shape, (name, H.shape)
    t = P.trial_values(FINEST, x, b.dirs["trial"], W.TRIAL_STEP, c, z0)
    r = W.ratios(ref, F=F, slack=slack, f0=y, f1=g, f2=H)
    rt = W.ratios(ref_t, f0=t["y"], f1=t["g"])
    tag = f"wall {name} [f2 {kind_f2}, other {kind_other}]"
    record_observation(f"{tag} error/bound: {_fmt(r)}; trial: {_fmt(rt)}; near the wall (k >= {W.NEAR_K}): "
                       + ", ".join(f"{k} {v[1]:.3f}" for k, v in r.items() if k != "f0"))
    assert np.all(np.isfinite(F)) and np.isfinite(y) and np.all(np.isfinite(g)) and np.all(np.isfinite(H)), name
    for what, (worst, _) in r.items():
        assert worst <= 1.0, (name, what, worst)
    assert np.array_equal(t["xn"], xt), name
    assert t["moved"] == 1 and t["finite"] == 1, (name, t["moved"], t["finite"])
    for what, (worst, _) in rt.items():
        assert worst <= 1.0, (name, "trial", what, worst)
    # f2: bitwise symmetric, and a fixed summation order
    assert np.array_equal(H, H.T), (name, np.argwhere(H != H.T)[:4])
    assert np.array_equal(np.asarray(P.f2(FINEST, x, c, z0).todense()), H), name
    # outside the cone: +inf, not NaN, at exactly the nodes outside; everything else as before
    Fo = P.node_barrier(xo)
    assert np.all(np.isposinf(Fo[b.out_nodes])), (name, Fo[b.out_nodes])
    ro = W.ratios(ref_o, F=Fo)
    assert ro["F"][0] <= 1.0, (name, "outside", ro)
    assert np.isposinf(P.f0(FINEST, xo, c, z0)), name
    to = P.trial_values(FINEST, x, b.dirs["outside"], W.TRIAL_STEP, c, z0)
    assert np.array_equal(to["xn"], xo), name
    assert to["finite"] == 0 and to["moved"] == 1, (name, to["finite"], to["moved"], to["y"])
