"""Every element-kernel variant (csrc/elem_kernels.hpp) at its dispatch and workgroup edges (DESIGN.md "Element-kernel
dispatch"): the hand-built problems of tests/elem_cases.py on the device.  Each test first asserts through
DeviceProblem.elem_plan that the modes it uses run the kernel the case names (and, for trials, the path bits), then holds the
numbers to the componentwise bounds of elem_cases.py.  The worst error / bound per case is recorded
(helpers.record_observation); no assertion is tuned from it."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import elem_cases as E
from gate_cases import KERNEL_RTOL
from helpers import record_observation

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN_KEYS = ("kind", "NY", "P", "threads", "G", "EPB", "grid", "lds", "nstage", "unstaged", "ymask")
_live = {}


def open_case(name):
    from mgb_amd.device import DeviceProblem, HipContext
    b = E.built(name)
    ctx = HipContext(0)
    P = DeviceProblem(ctx, b.M, b.Q, feasibility=b.case.phase1, NC=b.case.NC, barrier_weights=b.bw)
    if b.case.phase1:
        P.set_box(*b.box)
    return ctx, P


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for ctx, P in _live.values():
        P.close()
        ctx.close()
    _live.clear()


def device(name):
    if name not in _live:
        for ctx, P in _live.values():            # one resident problem at a time
            P.close()
            ctx.close()
        _live.clear()
        _live[name] = open_case(name)
    return _live[name][1]


def assert_plan(P, name, modes):
    """The kernel each mode runs, before any number: kind, instantiation, workgroup shape, grid, LDS, staging, ymask."""
    for mode in modes:
        got, want = P.elem_plan(mode), E.expected_plan(name, mode)
        assert {k: got[k] for k in PLAN_KEYS} == {k: want[k] for k in PLAN_KEYS}, (name, mode, got, want)
        assert got["newton_kind"] == got["kind"], (name, mode, got)
    return P.elem_plan(modes[-1])["kind"]


def assert_level(P, name, level):
    lp = P.level_plan(level)
    if level == 1:
        assert lp["R_unit"] and not lp["T_long"] and lp["T_chunks"] == 0, (name, lp)
    else:
        assert not lp["R_unit"] and lp["T_long"] == (E.CASE[name].n > 64) and lp["T_chunks"] == 0, (name, lp)
    return lp


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _id(v):
    return v if isinstance(v, str) else str(v)


def _tag(name, level, kind):
    return f"elem {name}/L{level} [{kind}]"


@pytest.mark.parametrize("name,level", E.LEVELS, ids=_id)
def test_node_maps(name, level):
    """z0 + R s and every row of Dz bit for bit, F and the slack against the oracle."""
    P = device(name)
    kind = assert_plan(P, name, ("node_F", "node_slack"))
    b = E.built(name)
    s, c, z0 = E.inputs(name, level)
    ev = E.element_eval(name, level)
    z_ref = z0 + b.R[level] @ s
    z = P.prolong_add(level, P.vec(s), P.vec(z0)).to_host()
    assert np.array_equal(z, z_ref)
    F, Dz = P.node_barrier(z, want_Dz=True)
    assert np.array_equal(Dz, ev["Dz"]), (name, level, np.argwhere(Dz != ev["Dz"])[:4])
    inside = np.ones(b.case.n, dtype=bool)
    inside[b.outside] = False
    e_F = rel(F[inside], ev["F"][inside])
    e_s = 0.0
    if ev["slack"] is not None:
        sl = P.node_slack(z)
        fin = inside & np.isfinite(ev["slack"])              # a node with every piece deselected has slack -Inf, on both sides
        assert np.array_equal(sl[inside & ~fin], ev["slack"][inside & ~fin]), (name, level)
        e_s = rel(sl[fin], ev["slack"][fin])
    record_observation(f"{_tag(name, level, kind)} Dz bitwise; node_barrier / node_slack: relative error {e_F:.2e} / {e_s:.2e} (asserted 1e-12)")
    assert e_F <= 1e-12 and e_s <= 1e-12, (name, level, e_F, e_s)


@pytest.mark.parametrize("name,level", E.LEVELS, ids=_id)
def test_f0_and_f1(name, level):
    P = device(name)
    kind = assert_plan(P, name, ("f0", "f1"))
    assert_level(P, name, level)
    s, c, z0 = E.inputs(name, level)
    f0, _ = E.f0_reference(name, level)
    y = P.f0(level, s, c, z0)
    e0 = abs(y - f0) / abs(f0)
    ref = E.f1_reference(name, level)
    g = P.f1(level, s, c, z0)
    r = ref.ratios(g)
    record_observation(f"{_tag(name, level, kind)} f0: relative error {e0:.2e} (asserted {KERNEL_RTOL:.0e}); f1: max error/bound {r.max():.3e}, "
                       f"skipped {ref.skipped:.3f}")
    assert np.isfinite(y) and np.all(np.isfinite(g)), (name, level)
    assert e0 <= KERNEL_RTOL, (name, level, e0)
    assert r.max() <= 1.0, (name, level, r.max())


@pytest.mark.parametrize("name,level", E.LEVELS, ids=_id)
def test_f2(name, level):
    P = device(name)
    kind = assert_plan(P, name, ("f2",))
    assert_level(P, name, level)
    s, c, z0 = E.inputs(name, level)
    ref = E.f2_reference(name, level)
    H = np.asarray(P.f2(level, s, c, z0).todense())
    assert H.shape == ref.value.shape and np.all(np.isfinite(H)), (name, level)
    assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max(), (name, level)
    r = ref.ratios(H)
    record_observation(f"{_tag(name, level, kind)} f2: max error/bound {r.max():.3e}, skipped {ref.skipped:.3f}")
    worst = np.unravel_index(np.argmax(np.abs(H - ref.value) / np.where(ref.bound > 0, ref.bound, np.inf)), H.shape)
    assert r.max() <= 1.0, (name, level, r.max(), worst)
    H2 = np.asarray(P.f2(level, s, c, z0).todense())
    assert np.array_equal(H, H2), (name, level)                                     # fixed summation order


def exact_step(x, d, step):
    """x - step d formed exactly and rounded once: what launch_step and the fused kernels promise (one fma)."""
    return np.array([float(Fraction(float(a)) - Fraction(float(step)) * Fraction(float(v))) for a, v in zip(x, d)])


def still_step(x, d):
    """A step so small that no entry of x changes: below a quarter of the spacing of every entry, derived from x and d."""
    assert np.all(x[d != 0] != 0)
    return float(np.min(np.spacing(np.abs(x[d != 0])) / (4.0 * np.abs(d[d != 0]))))


def check_trial(name, level, t, tag):
    b = E.built(name)
    x, d = b.s[level], b.dirs[level]
    assert np.array_equal(t["xn"], exact_step(x, d, E.TRIAL_STEP)) and np.array_equal(t["xn"], E.point(b, level, "trial")), (name, level)
    assert t["moved"] == 1 and t["finite"] == 1, (name, level, t["moved"], t["finite"])
    f0, _ = E.f0_reference(name, level, "trial")
    e0 = abs(t["y"] - f0) / abs(f0)
    ref = E.f1_reference(name, level, "trial")
    r = ref.ratios(t["g"])
    record_observation(f"{tag} trial y: relative error {e0:.2e} (asserted {KERNEL_RTOL:.0e}); trial g: max error/bound {r.max():.3e}, "
                       f"skipped {ref.skipped:.3f}")
    assert e0 <= KERNEL_RTOL, (name, level, e0)
    assert r.max() <= 1.0, (name, level, r.max())


@pytest.mark.parametrize("name,level", E.LEVELS, ids=_id)
def test_trial(name, level):
    """One line-search trial through the Newton loop's own trial_values: at the finest level the element kernel forms the
    trial point on the fly and the restriction runs fused with the step; at the coarse level (dense columns of R) neither."""
    P = device(name)
    kind = assert_plan(P, name, ("f01",))
    lp = assert_level(P, name, level)
    b = E.built(name)
    s, c, z0 = E.inputs(name, level)
    x, d = b.s[level], b.dirs[level]
    t = P.trial_values(level, x, d, E.TRIAL_STEP, c, z0)
    assert t["on_the_fly"] == (level == 1), (name, level, t["on_the_fly"])
    assert t["fused_restrict"] == (not lp["T_long"]), (name, level, t["fused_restrict"])
    if E.CASE[name].n > 64:
        assert t["fused_restrict"] == (level == 1)
    check_trial(name, level, t, _tag(name, level, kind))
    # the same point through f0 / f1: both are held to the reference; bitwise equality is recorded, not asserted
    same_y = P.f0(level, t["xn"], c, z0) == t["y"]
    same_g = np.array_equal(P.f1(level, t["xn"], c, z0), t["g"])
    record_observation(f"{_tag(name, level, kind)} trial bitwise equal to f0 / f1 at the same point: {same_y} / {same_g}")
    # a step too small to change any entry: the stamp of the step kernel is not raised
    t0 = P.trial_values(level, x, d, still_step(x, d), c, z0)
    assert np.array_equal(exact_step(x, d, still_step(x, d)), x)
    assert t0["moved"] == 0 and t0["finite"] == 1 and np.array_equal(t0["xn"], x), (name, level, t0["moved"])
    # an ordinary step again (the stamp moves on), then a trial point outside the cone: rejected, not an error
    assert P.trial_values(level, x, d, E.TRIAL_STEP, c, z0)["moved"] == 1
    if b.case.slack_states and not b.case.masked:
        n = b.case.n
        z = z0 + b.R[level] @ x
        zd = b.R[level] @ d
        a = b.case.slack_states[0]
        sl, sd = z[a * n:(a + 1) * n], zd[a * n:(a + 1) * n]
        assert np.any(sd > 0) or b.case.N == 1               # (the two nodes of the one-element case both move inward at level 0)
        if np.any(sd > 0):
            big = 2.0 * float(np.max(sl[sd > 0] / sd[sd > 0]))       # the slack of at least one node becomes negative
            tb = P.trial_values(level, x, d, big, c, z0)
            assert tb["finite"] == 0 and tb["moved"] == 1, (name, level, tb["finite"], tb["y"])


def _worker(tmp_path, what, name, env):
    out = str(tmp_path / f"{what}_{name}_{'_'.join(sorted(env)) or 'default'}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "elem_trial_worker.py"), out, what, name], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr
    return np.load(out)


@pytest.mark.parametrize("name", E.WORKER_CASES)
@pytest.mark.parametrize("switch", ["MGBHIP_NO_FUSED_STEP", "MGBHIP_NO_FUSED_RESTRICT"])
def test_trial_without_the_fused_branches(tmp_path, name, switch):
    """The finest level with the step kernel in front of the evaluation / the separate restriction: same bounds."""
    d = _worker(tmp_path, "trial", name, {switch: "1"})
    plan = json.loads(str(d["plan"]))
    want = E.expected_plan(name, "f01")
    assert {k: plan[k] for k in PLAN_KEYS} == {k: want[k] for k in PLAN_KEYS}, (name, plan, want)
    moved, finite, onfly, fused = (int(v) for v in d["flags"])
    assert (onfly, fused) == ((0, 1) if switch == "MGBHIP_NO_FUSED_STEP" else (1, 0)), (name, switch, onfly, fused)
    t = dict(y=float(d["y"]), g=d["g"], xn=d["xn"], moved=moved, finite=finite)
    check_trial(name, 1, t, f"elem {name}/L1 [{plan['kind']}, {switch}=1]")


# ---- the condensing f2 on real fem2d_P2 meshes -------------------------------------------------------------------------------

def strip_mesh(nt):
    """nt P2 + bubble triangles in a strip over [-1, 1] x [0, 1]: corners in slots 0, 2, 4, edge midpoints, centroid."""
    K = np.zeros((7, nt, 2))
    for t in range(nt):
        i = t // 2
        a, b, c = ((i, 0.0), (i + 1, 0.0), (i, 1.0)) if t % 2 == 0 else ((i + 1, 0.0), (i + 1, 1.0), (i, 1.0))
        a, b, c = (np.array(v, dtype=np.float64) for v in (a, b, c))
        K[:, t, :] = [a, (a + b) / 2, b, (b + c) / 2, c, (c + a) / 2, (a + b + c) / 3]
    K[:, :, 0] = K[:, :, 0] * (2.0 / ((nt + 1) // 2)) - 1.0
    return K


CONDENSE_MESHES = {"L2": 8, "L3": 32, "strip33": 33}          # elements: a partial workgroup, exactly one, one plus one element


def condense_problem(mesh):
    import mgb_amd as m
    geom = m.fem2d_P2(K=strip_mesh(33)) if mesh == "strip33" else m.subdivide(m.fem2d_P2(), int(mesh[1:]))
    return m.assemble(m.amg(geom), p=1.5)


def condense_run(prob):
    """Two Newton directions at the finest level (the first call assembles, the second runs the condensing kernel where the
    level has condensed leaves) against the oracle's system: normwise backward error and lambda^2."""
    import scipy.sparse as sp
    from mgb_amd.device import DeviceMGBProblem
    from oracle import mgb_oracle as O
    D = DeviceMGBProblem(prob, device_id=0)
    P = D.main
    Mo = O.OracleAMG(prob.M[0])
    B = O.Barrier(prob.Q)
    J = len(Mo.R_fine) - 1
    R = Mo.R_fine[J]
    z0 = np.ascontiguousarray(prob.g.T).reshape(-1)
    c = 0.1 * prob.f
    s = 1e-3 * np.random.default_rng(5).standard_normal(R.shape[1])
    g_o = B.f1(s, Mo.w, c, R, Mo.D_fine, z0)
    H_o = sp.csr_matrix(B.f2(s, Mo.w, c, R, Mo.D_fine, z0))
    hn, gn = float(abs(H_o).sum(axis=1).max()), float(np.linalg.norm(g_o, np.inf))
    before = P.elem_plan("f2")
    bwd, lam_err, conds = [], [], []
    for _ in range(2):
        x, lam, cond = P.newton_direction(J, s, c, z0)
        conds.append(int(cond))
        bwd.append(float(np.linalg.norm(H_o @ x - g_o, np.inf) / (hn * np.linalg.norm(x, np.inf) + gn)))
        lam_err.append(abs(lam - float(g_o @ x)) / abs(lam))
    after = P.elem_plan("f2")
    out = dict(N=P.N, grid=after["grid"], EPB=after["EPB"], kind_before=before["newton_kind"], kind_after=after["newton_kind"],
               plain_kind=after["kind"], conds=np.array(conds), bwd=np.array(bwd), lam=np.array(lam_err))
    D.close()
    return out


def check_condense(mesh, d, tag):
    N = CONDENSE_MESHES[mesh]
    assert int(d["N"]) == N and int(d["EPB"]) == 32 and int(d["grid"]) == -(-N // 32), (mesh, d["N"], d["grid"])
    assert str(d["plain_kind"]) == "fast_default" and str(d["kind_before"]) == "fast_default", (mesh, d["plain_kind"], d["kind_before"])
    record_observation(f"elem condense {mesh} N={N} {tag}: newton_kind {d['kind_after']}, condensed {[int(v) for v in d['conds']]}, direction backward "
                       f"error {max(d['bwd']):.1e}, lambda^2 {max(d['lam']):.1e} (asserted {KERNEL_RTOL:.0e})")
    assert str(d["kind_after"]) == "condense" and list(d["conds"]) == [0, 1], (mesh, d["kind_after"], d["conds"])
    assert max(d["bwd"]) <= KERNEL_RTOL and max(d["lam"]) <= KERNEL_RTOL, (mesh, d["bwd"], d["lam"])


@pytest.mark.parametrize("mesh", list(CONDENSE_MESHES))
def test_condensing_f2_at_workgroup_edges(mesh):
    for ctx, P in _live.values():
        P.close()
        ctx.close()
    _live.clear()
    check_condense(mesh, condense_run(condense_problem(mesh)), "packed leaves")


@pytest.mark.parametrize("mesh", list(CONDENSE_MESHES))
def test_condensing_f2_with_square_leaves(tmp_path, mesh):
    check_condense(mesh, _worker(tmp_path, "condense", mesh, {"MGBHIP_NO_PACKED_LEAVES": "1"}), "MGBHIP_NO_PACKED_LEAVES=1")
