"""Every shape-gated transfer, reduction and assembly kernel at its gate (DESIGN.md "Shape gates"): the hand-built hierarchies
of tests/gate_cases.py on the device.  Each test first asserts through DeviceProblem.level_plan that the level took the kernel
the case was built for -- a case that slips to the other side of a gate fails -- and then holds the result to the componentwise
bound of gate_cases.py against the exact reference.  The worst error / bound per kernel variant is recorded
(helpers.record_observation); no assertion is tuned from it."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import gate_cases as G
from helpers import record_observation

pytestmark = pytest.mark.gpu

KERNEL_RTOL = G.KERNEL_RTOL
TRANSFER_KEYS = ("R_unit", "R_long", "T_long", "T_chunks", "max_row", "max_col")
HERE = os.path.dirname(os.path.abspath(__file__))
_live = {}


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for ctx, P in _live.values():
        P.close()
        ctx.close()
    _live.clear()


def device(name):
    from mgb_amd.device import DeviceProblem, HipContext
    if name not in _live:
        for ctx, P in _live.values():            # one resident hierarchy at a time
            P.close()
            ctx.close()
        _live.clear()
        prob = G.problem(name)
        ctx = HipContext(0)
        _live[name] = (ctx, DeviceProblem(ctx, prob.M[0], prob.Q))
    return _live[name][1]


def _assert_plan(plan, expect, keys=None):
    for key in (keys or expect):
        assert plan[key] == expect[key], (key, plan[key], expect[key], plan)


def _id(v):
    return v if isinstance(v, str) else str(v)


@pytest.mark.parametrize("name,level", G.op_params("prolong"), ids=_id)
def test_prolongation(name, level):
    lv = G.CASE[name].all_levels()[level]
    P = device(name)
    plan = P.level_plan(level)
    _assert_plan(plan, lv.expect, TRANSFER_KEYS)
    s, c, z0 = G.inputs(name, level)
    ref = G.prolong_reference(name, level)
    z = P.prolong_add(level, P.vec(s), P.vec(z0)).to_host()
    r = ref.ratios(z)
    record_observation(f"gate prolong_add {name}/{lv.name} (longest row {plan['max_row']}): max error/bound {r.max():.3f}")
    assert r.max() <= 1.0, (name, lv.name, r.max())
    # z0 + R s as the element kernels read it: fused selection read (R_unit), prolong_kernel, or wave per row (R_long)
    variant = "fused selection read" if plan["R_unit"] else "wave per row" if plan["R_long"] else "prolong_kernel"
    y_o = G.oracle_f0(name, level)
    err = abs(P.f0(level, s, c, z0) - y_o) / abs(y_o)
    record_observation(f"gate f0 through {variant} {name}/{lv.name}: relative error {err:.2e} (asserted {KERNEL_RTOL:.0e})")
    assert err <= KERNEL_RTOL, (name, lv.name, variant, err)


@pytest.mark.parametrize("name,level", G.op_params("restrict"), ids=_id)
def test_restriction(name, level):
    lv = G.CASE[name].all_levels()[level]
    P = device(name)
    plan = P.level_plan(level)
    _assert_plan(plan, lv.expect, TRANSFER_KEYS)
    ref = G.restrict_reference(name, level)
    g = P.f1(level, *G.inputs(name, level))
    r = ref.ratios(g)
    variant = f"chunked x{plan['T_chunks']}" if plan["T_chunks"] else "wave per row" if plan["T_long"] else "thread per row"
    record_observation(f"gate restriction {variant} {name}/{lv.name} (longest column {plan['max_col']}, {g.size} columns): "
                       f"max error/bound {r.max():.3e}")
    assert r.max() <= 1.0, (name, lv.name, variant, r.max())


def _check_assembly(name, level, Hflat, plan, expect, tag):
    m = G.level_R(name, level).shape[1]
    ref = G.assemble_reference(name, level)
    H = Hflat.reshape(m, m)
    assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max(), (name, level, tag)         # symmetry, as tests/test_gpu_parity.py
    r = ref.ratios(Hflat)
    variant = plan["projection"] + (" + two-stage gather" if plan["gather_nchunk"] > 1 else " + wave gather" if plan["long_lists"]
                                    else "" if plan["acc"] else " + thread gather")
    record_observation(f"gate assembly {variant} {name}/{G.CASE[name].all_levels()[level].name}{tag}: max error/bound {r.max():.3e}")
    assert r.max() <= 1.0, (name, level, tag, variant, r.max())
    # nothing outside the structural pattern of the reference's upper triangle and its mirror
    mask = np.zeros(m * m, dtype=bool)
    if m <= G.ALL_BELOW:
        mask[ref.index] = True
        mask |= mask.reshape(m, m).T.reshape(-1)
        assert np.all(Hflat[~mask] == 0.0), (name, level, tag)


@pytest.mark.parametrize("name,level", G.op_params("assemble"), ids=_id)
def test_assembly(name, level):
    lv = G.CASE[name].all_levels()[level]
    P = device(name)
    H = P.f2(level, *G.inputs(name, level))
    plan = P.level_plan(level)
    assert plan["planned"]
    _assert_plan(plan, lv.expect)
    _check_assembly(name, level, G.dense_H(H, H.shape[0]), plan, lv.expect, "")


SWITCHED = [(c.name, l, env, proj) for c in G.CASES for l, lv in enumerate(c.all_levels()) for env, proj in lv.switches]


@pytest.mark.parametrize("name,level,env,projection", SWITCHED, ids=_id)
def test_assembly_under_a_kernel_switch(name, level, env, projection, tmp_path):
    """The same level through the kernel that an environment switch selects (read once per process: a worker process)."""
    lv = G.CASE[name].all_levels()[level]
    out = str(tmp_path / "H.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gate_cases.py"), "assemble", name, str(level), out],
                       capture_output=True, text=True, timeout=300, env=dict(os.environ, **{env: "1"}))
    assert r.returncode == 0, r.stdout + r.stderr
    data = np.load(out)
    plan = json.loads(str(data["plan"]))
    _assert_plan(plan, dict(lv.expect, projection=projection))
    _check_assembly(name, level, data["H"], plan, lv.expect, f" [{env}=1]")


# ---- vector reductions ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from mgb_amd.device import HipContext
    c = HipContext(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", G.reduction_lengths())
def test_vector_reductions(ctx, n):
    """dot / norm / all_isfinite against math.fsum of exactly formed products (entries of <= 26 significant bits), bound
    (n + 1) 2^-53 sum |a_i b_i| (one more rounding for the square root); axpy / scale / fill / copy bit for bit."""
    from mgb_amd.device import DeviceVector
    a, b = G.reduction_vectors(n)
    da, db = DeviceVector(ctx, a), DeviceVector(ctx, b)
    dot_ref, dot_abs = math.fsum((a * b).tolist()), math.fsum(np.abs(a * b).tolist())
    e_dot = abs(da.dot(db) - dot_ref) / ((n + 1) * G.U53 * dot_abs)
    sq = math.fsum((a * a).tolist())
    # |sqrt(S (1 + d)) (1 + e) - sqrt(S)| <= sqrt(S) (d / 2 + e), d <= (n + 1) u, e <= u
    e_norm = abs(da.norm() - math.sqrt(sq)) / (math.sqrt(sq) * ((n + 1) * G.U53 / 2 + 2 * G.U53))
    record_observation(f"gate reductions n={n}: dot error/bound {e_dot:.3f}, norm error/bound {e_norm:.3f}")
    assert e_dot <= 1.0 and e_norm <= 1.0, (n, e_dot, e_norm)
    assert da.all_isfinite()
    B = G.reduce_block_cap()
    for pos in sorted({0, n - 1, min(n - 1, 256), min(n - 1, 255), min(n - 1, 256 * B), min(n - 1, 256 * B - 1)}):
        for bad in (np.nan, np.inf, -np.inf):
            v = a.copy()
            v[pos] = bad
            assert not DeviceVector(ctx, v).all_isfinite(), (n, pos, bad)
    alpha = 0.3984375
    assert np.array_equal(da.copy().to_host(), a)
    assert np.array_equal(da.copy().axpy(alpha, db).to_host(), a + alpha * b)      # alpha b_i is exact (6 + 26 bits): fused or not
    assert np.array_equal((da * alpha).to_host(), a * alpha)
    assert np.array_equal(DeviceVector(ctx, length=n).fill(-2.5).to_host(), np.full(n, -2.5))
    assert da.n == n and np.array_equal(da.to_host(), a)              # the operands are untouched


# ---- a complete solve on a hierarchy whose coarsest restriction is chunked --------------------------------------------------

def _solve(tmp_path, tag, env):
    out = str(tmp_path / f"{tag}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "gate_cases.py"), "solve", out], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout + r.stderr
    d = np.load(out)
    for plan, expect in zip(json.loads(str(d["plans"])), G.SOLVE_PLANS, strict=True):
        _assert_plan(plan, expect)
    return d["z"], d["its"]


def test_trial_fusion_switches_are_bitwise_on_a_chunked_restriction_level(tmp_path):
    """tests/test_gpu_solver_switches.py on a hierarchy whose level 0 restricts through the chunked kernel (columns of 2048
    entries) and whose level 1 through the row-parallel one: mgb_solve to convergence with and without the fused restriction
    of a line-search trial and the fused step -- the same z and the same iteration counts, bit for bit."""
    z0, its0 = _solve(tmp_path, "default", {})
    assert np.all(np.isfinite(z0)) and its0.sum() > 0
    for sw in ("MGBHIP_NO_FUSED_RESTRICT", "MGBHIP_NO_FUSED_STEP"):
        z, its = _solve(tmp_path, sw, {sw: "1"})
        assert np.array_equal(z, z0) and np.array_equal(its, its0), sw
