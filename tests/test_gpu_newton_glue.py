"""The glue of the Newton loop, new path against old path, bit for bit (-m gpu): the finishing launch that sums all its jobs at
once (MGBHIP_FINISH_SERIAL=1: one after another), the start point of a Newton solve from one pass over the elements
(MGBHIP_SPLIT_START=1: f0, f1 and vec_stats with two read-backs) and the level solves that read z in place
(MGBHIP_Z_SNAPSHOT=1: from a copy).  None of the three changes a floating-point operation or its order, so every comparison
here is np.array_equal.

The switches are read once per process: tests/newton_glue_worker.py runs each configuration in a process of its own (at most
once per session) and the tests compare the files it leaves."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import gate_cases as G
import newton_glue_worker as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_TMP = tempfile.TemporaryDirectory(prefix="newton_glue_")


# what each configuration is asked for: one process per configuration
PARTS = {"old": "solves edges record reject snapshot", "finish": "solves edges", "start": "solves record reject",
         "snapshot": "solves snapshot", "new": "solves record reject snapshot", "levels": "levels"}
LEVELS_ENV = ("MGBHIP_NO_FUSED_STEP", "MGBHIP_NO_FUSED_RESTRICT")      # "levels": the new paths, the trial's fused branches off


@functools.lru_cache(maxsize=None)
def run(config):
    """The worker's output for PARTS[config] with the old-path switches of `config` set."""
    env = {k: v for k, v in os.environ.items() if k not in W.SWITCHES + LEVELS_ENV}
    env.update({k: "1" for k in (LEVELS_ENV if config == "levels" else W.CONFIGS[config])})
    out = os.path.join(_TMP.name, f"{config}.npz")
    r = subprocess.run([sys.executable, os.path.join(HERE, "newton_glue_worker.py"), out] + PARTS[config].split(), capture_output=True,
                       text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with np.load(out) as f:
        return {k: f[k] for k in f.files}


def same(a, b, prefix):
    keys = sorted(k for k in a if k.startswith(prefix))
    assert keys and keys == sorted(k for k in b if k.startswith(prefix)), prefix
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), k


# ---- whole solves ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["finish", "start", "snapshot", "new"])
@pytest.mark.parametrize("name", W.SOLVES)
def test_whole_solve_is_bitwise_the_old_path(name, config):
    """z, its, ts, kappas, c_dot_Dz and the f0 / f1 / f2 / factorization counters of the main phase (and of phase I where it
    runs): each new path alone and all three together against all three switched off."""
    old, new = run("old"), run(config)
    assert bool(old[f"solve/{name}/phase1"]) == (name == "phase1")
    assert int(old[f"solve/{name}/main/newton_iterations"]) > 0
    same(old, new, f"solve/{name}/")


# ---- the finishing sums at their edges ---------------------------------------------------------------------------------

@pytest.mark.parametrize("N", W.edge_elements())
def test_finishing_sums_at_count_edges(N):
    """f0, a line-search trial (job 0: the f0 partials, ceil(N / 128) of them; jobs 1, 2: the reduction's workgroups) and a
    Newton direction (three jobs of reduce_blocks(m) partials), finish_kernel<U> against the serial kernel."""
    old, new = run("old"), run("finish")
    assert int(new[f"edge/{N}/grid"]) == -(-N // W.EPB) and int(new[f"edge/{N}/m"]) == 3 * N - 1
    assert np.array_equal(new[f"edge/{N}/trial_flags"], [1, 1])
    assert (f"edge/{N}/dir_lambda2" in new) == (N in W.DIRECTION_N)
    same(old, new, f"edge/{N}/")


def test_finishing_sum_edges_are_the_ones_meant():
    U = W.finish_loads_in_flight()
    cap = G.reduce_block_cap()
    counts = {-(-N // W.EPB) for N in W.edge_elements()}
    assert {1, 255, 256, 257, 256 * U - 1, 256 * U, 256 * U + 1, 3 * 256 * U + 5} <= counts
    blocks = {min(-(-(3 * N - 1) // 256), cap) for N in W.DIRECTION_N}
    assert blocks == {1, 2, cap - 1, cap} and 3 * 87424 - 1 > 256 * cap


# ---- the start point ---------------------------------------------------------------------------------------------------

EXPECT_PLAN = {("restrict_cols", 1): (0, 0, 0), ("restrict_cols", 2): (0, 1, 0), ("restrict_cols", 3): (0, 1, 0), ("restrict_cols", 4): (0, 1, 1),
               ("restrict_cols", 0): (0, 1, 3), ("restrict_cols", 9): (1, 0, 0), ("prolong_rows", 1): (0, 1, 0)}


@pytest.mark.parametrize("case,level", W.START_LEVELS)
def test_start_sequence_is_bitwise_f0_and_f1(case, level):
    """The start point's launches (f01 element kernel at a stored point, eval_f1's restriction, block_reduce<1>, one finishing
    launch) against f0 and f1 at the same point: on a thread-per-row level, wave-per-row levels, the chunked restriction at
    its gate (1023 / 1024) and beyond, and the selection level.  The sequence is reached through a line-search trial with
    step 0 and the trial's fused branches off (the only public evaluation that runs it outside a solve)."""
    d = run("levels")
    tag = f"level/{case}/{level}"
    assert tuple(d[f"{tag}/plan"]) == EXPECT_PLAN[(case, level)]
    assert np.array_equal(d[f"{tag}/path"], [0, 0, 1]) and not d[f"{tag}/trial_x"].any()
    assert np.isfinite(d[f"{tag}/f0"]) and np.array_equal(d[f"{tag}/trial_y"], d[f"{tag}/f0"])
    assert np.array_equal(d[f"{tag}/trial_g"], d[f"{tag}/f1"])


@pytest.mark.parametrize("name", ["p2_L3_p1", "gate_solve"])
def test_start_values_inside_a_solve(name):
    """Every call of the stopping rule in a whole solve, old start against new: the first call of each Newton solve carries the
    start point's y (ymin) and |g| = sqrt(|g|^2) (gmin), the later ones everything that followed from them."""
    old, new = run("old"), run("start")
    calls = new[f"record/{name}/calls"]
    assert calls.shape[0] > 10 and np.all(np.isfinite(calls[:, [0, 2]]))
    same(old, new, f"record/{name}/")
    same(old, run("new"), f"record/{name}/")


@pytest.mark.parametrize("config", ["start", "new"])
def test_infeasible_start_is_rejected_as_before_and_the_next_solve_is_unharmed(config):
    old, new = run("old"), run(config)
    assert "newton: initial objective value is not finite" in str(new["reject/message"])
    assert str(new["reject/message"]) == str(old["reject/message"])
    assert int(new["reject/status"]) == 0
    same(old, new, "reject/")
    for k in ("z", "its", "ts", "kappas", "c_dot_Dz", "f0_evals", "f1_evals", "f2_evals", "factorizations"):
        assert np.array_equal(new[f"reject/next/{k}"], old[f"solve/fem1d/main/{k}"]), k


# ---- no snapshot of z --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("config", ["snapshot", "new"])
def test_recursing_and_failing_steps_without_the_snapshot(config):
    old, new = run("old"), run(config)
    # a) level attempts that fail and recurse, t-steps that fail and are repeated with a smaller kappa
    its, kappas = new["snapshot/recurse/its"], new["snapshot/recurse/kappas"]
    assert int(new["snapshot/recurse/status"]) != 0 and kappas[0] == 10.0 and np.all(kappas[1:] < 10.0)
    assert np.all(its[:-1].sum(axis=1) > 0), "the coarse levels are reached only by recursion"
    same(old, new, "snapshot/recurse/")
    # b) z after t-steps that failed (one of them after a converged level solve had been prolonged into z) is the iterate the
    #    ramp started from
    seen = new["snapshot/rollback/seen"]
    assert int(new["snapshot/rollback/status"]) != 0 and int(new["snapshot/rollback/failure_code"]) == 1
    assert bool(new["snapshot/rollback/said_yes"]) and seen.shape[0] == 2
    assert np.array_equal(seen[0], seen[1]) and np.array_equal(new["snapshot/rollback/z"], seen[0])
    assert float(new["snapshot/rollback/kappas"][1]) <= 1.0 and int(new["snapshot/rollback/its"][1, 1]) > 0
    same(old, new, "snapshot/rollback/")
