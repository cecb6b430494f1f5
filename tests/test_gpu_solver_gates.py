"""Every shape-gated kernel of the sparse LDL' at its gate (DESIGN.md "Solver shape gates"): the hand-built levels of
tests/solver_gate_cases.py on the device.  Each case first asserts through DeviceProblem.solver_launches that its fronts took the
kernels the case was built for -- a case that slips across its gate fails there -- and then holds both solve paths to the
project's componentwise backward-error bar with an exactly formed residual.  The worst eta / ETA_MAX per kernel variant is
recorded (helpers.record_observation); no assertion is tuned from it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_gate_cases as S
from helpers import record_observation
from test_gpu_solver import ETA_MAX

assert S.ETA_MAX == ETA_MAX, "tests/solver_gate_cases.py must carry the project's bar of tests/test_gpu_solver.py unchanged"

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_live = {}


@pytest.fixture(scope="module")
def device():
    from mgb_amd.device import DeviceProblem, HipContext
    prob = S.problem()
    ctx = HipContext(0)
    P = DeviceProblem(ctx, prob.M[0], prob.Q)         # the one resident hierarchy of this module
    yield P
    P.close()
    ctx.close()


def variant(r):
    """The factorization kernel of a launch row, as the observations name it."""
    if r["tiny"]:
        return "mf_factor_tiny" + (" packed" if r["packed"] else "")
    if r["wave"]:
        return "mf_factor_wave<%d>" % (32 if r["cls"] <= 32 else 48)
    if r["cls"]:
        return "mf_factor_small cls %d bwd %s" % (r["cls"], r["backward"])
    return "large %s/%s/%s" % ("inverse" if r["inv"] else "substitution", r["assembly"], r["block0"])


def check(name, res, rows, tag=""):
    assert bool(res[name + "_pattern_ok"]), (name, "the level's Hessian pattern is not the case's pattern")
    got = json.loads(str(res[name + "_rows"]))
    assert got == rows, (name, tag, got)                                   # (a) the plan, before any number is looked at
    worst = 0.0
    for grade in S.CASE[name].grades:
        A, g, _ = S.system(name, grade)
        x_ref = S.reference(name, grade)
        lam_ref = float(g @ x_ref)
        key = f"{name}_g{grade}"
        for suffix in ("_x", "_xn"):                                       # (b) forward + backward sweeps / bordered factorization
            x = res[key + suffix]
            assert np.isfinite(x).all(), (name, tag, grade, suffix)
            e = S.eta(A, x, g)
            print(f"{name}{tag} grade {grade} {suffix}: eta {e:.3e} = {e / ETA_MAX:.3e} ETA_MAX")
            worst = max(worst, e)
            assert e <= ETA_MAX, (name, tag, grade, suffix, e)
            assert np.array_equal(x, res[key + suffix + "_again"]), (name, tag, grade, suffix, "not bitwise reproducible")   # (c)
        lam, status = res[key + "_lam"]
        assert status == 0.0, (name, tag, grade, status)
        assert abs(lam - lam_ref) <= 1e-9 * abs(lam_ref), (name, tag, grade, lam, lam_ref)
        assert np.array_equal(res[key + "_lam"], res[key + "_lam_again"])
    # (d) eta is a property of the whole solve: the figure is per case, listed with every kernel variant the case ran
    record_observation(f"solver gate {name}{tag}: worst eta / ETA_MAX {worst / ETA_MAX:.3e} through "
                       + "; ".join(sorted({variant(r) for r in got})))


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_launch_plan_and_backward_error_at_the_gate(device, name):
    res = {}
    S.run_cases(device, [name], res)
    check(name, res, S.CASE[name].rows)


SWITCHED = [(c.name, env) for c in S.CASES for env in c.switched]


@pytest.mark.parametrize("name,env", SWITCHED, ids=lambda v: v if isinstance(v, str) else "+".join(f"{k}={x}" for k, x in v))
def test_the_same_case_under_a_kernel_switch(name, env, tmp_path):
    """(e) The switches are read once per process: a worker process per (case, switch)."""
    out = str(tmp_path / "res.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "solver_gate_cases.py"), out, name], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **dict(env)))
    assert r.returncode == 0, r.stdout + r.stderr
    check(name, dict(np.load(out)), S.CASE[name].switched[env], " [" + " ".join(f"{k}={x}" for k, x in env) + "]")


# ---- zero pivots inside each kernel family ---------------------------------------------------------------------------------

ZERO_TAGS = [z[0] for z in S.ZERO_PIVOTS]


def _check_fallback(tag, res):
    """As shipped: the pivoted LU takes over, both paths return H^-1 g to 1e-9 (the tolerance of
    test_zero_pivot_falls_back_to_the_pivoted_lu_like_the_reference) with status OK."""
    A, g, x_ref, _ = S.zero_pivot_system(tag)
    for suffix, st in (("_x", "_status"), ("_xn", "_statusn")):
        assert float(res[tag + st]) == 0.0, (tag, suffix, float(res[tag + st]))
        x = res[tag + suffix]
        assert np.isfinite(x).all() and np.linalg.norm(x - x_ref) <= 1e-9 * np.linalg.norm(x_ref), (tag, suffix)
    lam_ref = float(g @ x_ref)
    assert abs(float(res[tag + "_lam"]) - lam_ref) <= 1e-9 * max(abs(lam_ref), np.linalg.norm(g) * np.linalg.norm(x_ref) * 1e-3)


@pytest.mark.parametrize("tag", ZERO_TAGS)
def test_zero_pivot_inside_a_kernel_family_falls_back_to_the_pivoted_lu(device, tag):
    name = S.ZERO[tag][1]
    res = {}
    S.run_zero_pivots(device, [tag], res)
    assert device.solver_launches(S.LEVEL[name]) == S.CASE[name].rows
    _check_fallback(tag, res)


def test_zero_pivots_are_reported_by_every_kernel_family_without_the_fallback(tmp_path):
    """MGBHIP_NO_LU_FALLBACK=1 (one worker process for all placements): both solve paths return MGBHIP_ERR_NOT_SPD -- the
    kernel that met the pivot flagged it; no solve returns a finite answer with status OK."""
    from mgb_amd import device as dev
    out = str(tmp_path / "zero.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "solver_gate_cases.py"), out, "zero"] + ZERO_TAGS, capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, MGBHIP_NO_LU_FALLBACK="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    res = dict(np.load(out))
    for tag in ZERO_TAGS:
        assert float(res[tag + "_status"]) == dev.ERR_NOT_SPD, (tag, "solve", float(res[tag + "_status"]))
        assert float(res[tag + "_statusn"]) == dev.ERR_NOT_SPD, (tag, "solve_newton", float(res[tag + "_statusn"]))
