"""Threads per front of mf_factor_small by the launch (csrc/mf_launch_plan.hpp: factor_small_threads) against 256, 512 and
1024 threads for every launch of a class above 32 (MGBHIP_SMALL_THREADS).  The block size decides which thread owns an entry
of the front, never the order of the additions into it -- children stay ordered with a barrier between them, on both sides of
the `b * b <= threads` split between the one-entry-per-thread and the 2-D extend-add, and the update tiles are disjoint -- so
every comparison is bitwise.  Worker processes (the switch is read once per process): one per setting runs the gate cases of
tests/solver_gate_cases.py that have a launch of mf_factor_small above class 32, one per setting and refinement a whole solve.

The library has no read-back of the frontal arena; the factors are compared through what they determine, the generic solve
(forward and backward sweep over every factor entry) and the carried one (the factorization's own forward substitution), on
two gradings and twice each."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_gate_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"rule": {}, "t256": {"MGBHIP_SMALL_THREADS": "256"}, "t512": {"MGBHIP_SMALL_THREADS": "512"},
         "t1024": {"MGBHIP_SMALL_THREADS": "1024"}}
OTHERS = [p for p in PATHS if p != "t256"]
SWITCHES = ("MGBHIP_SMALL_THREADS", "MGBHIP_BORDER_LAUNCHES")


def _small(r):
    return r["cls"] >= 48 and not r["wave"] and not r["tiny"]


# every gate case with an mf_factor_small launch of a class above 32
CASES = [c.name for c in S.CASES if any(_small(r) for r in c.rows)]


def _worker(script, args, env, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(e, **env))
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """(kind, path) -> arrays of one worker: computed once, shared by the tests, never changed."""
    d = tmp_path_factory.mktemp("small_threads")
    cache = {}

    def get(kind, path):
        if (kind, path) not in cache:
            out = str(d / f"{kind}_{path}.npz")
            if kind == "gates":
                _worker("solver_gate_cases.py", [out] + CASES, PATHS[path])
            else:               # solve5, solve6
                _worker("gather_maps_worker.py", [out, kind[len("solve"):]], PATHS[path])
            cache[kind, path] = dict(np.load(out))
        return cache[kind, path]
    return get


def test_the_cases_hold_the_shapes_the_block_size_matters_for():
    """(level, m, k, children, how many) of the pinned plans.  A block arrow's leaf (k_i, k_i + s + 1) hands its parent an update
    block of b = s + 1 rows; the `b * b <= threads` split moves at 256, 512 and 1024."""
    fronts = {name: S.CASE[name].fronts for name in CASES}
    classes = {r["cls"] for name in CASES for r in S.CASE[name].rows if _small(r)}
    assert classes == {48, 64, 88, 128}, classes

    def child_rows(name):          # update-block sizes of the fronts that have a parent in an LDS launch
        return {m - k for (lev, m, k, nch, cnt) in fronts[name] if not (m == 1 and k == 1)}
    assert 6 in child_rows("leaf_lds")                                             # b * b <= 256 (packed tiny leaves, class-128 parent)
    assert 18 in child_rows("lds64") and 21 in child_rows("k8")                    # 256 < b * b <= 512
    assert 28 in child_rows("lds128") and 31 in child_rows("ch17")                 # 512 < b * b <= 1024
    assert 42 in child_rows("merge255") and 42 in child_rows("k17")                # above
    assert any(k % 8 for name in CASES for (_, m, k, _, _) in fronts[name])
    assert any(nch > 4 for name in ("merge255", "ch16", "ch17", "n1023", "leaf_lds") for (_, _, _, nch, _) in fronts[name])
    for name, cls in (("wave48", 48), ("lds64", 64), ("lds88", 88), ("lds128", 128)):       # m equal to the class
        assert any(m == cls and nch > 0 for (_, m, k, nch, _) in fronts[name]), name
    assert {"leaf_lds", "lds64", "k8", "lds128", "ch17", "merge255", "k17", "wave48", "lds88", "ch16", "n1023"} <= set(CASES)


@pytest.mark.parametrize("name", CASES)
def test_gate_case_has_its_rows_and_is_reproducible_at_256(results, name):
    a = results("gates", "t256")
    assert bool(a[name + "_pattern_ok"])
    assert json.loads(str(a[name + "_rows"])) == S.CASE[name].rows, name
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam"):
            key = f"{name}_g{grade}{suffix}"
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], a[key + "_again"]), key


@pytest.mark.parametrize("path", OTHERS)
@pytest.mark.parametrize("name", CASES)
def test_gate_case_is_bitwise_the_same_at_every_block_size(results, name, path):
    a, b = results("gates", "t256"), results("gates", path)
    assert bool(b[name + "_pattern_ok"])
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam", "_x_again", "_xn_again", "_lam_again"):
            key = f"{name}_g{grade}{suffix}"
            assert np.array_equal(a[key], b[key]), (key, path)


@pytest.mark.parametrize("path", OTHERS)
@pytest.mark.parametrize("L", [5, 6])
def test_whole_solve_is_bitwise_the_same_at_every_block_size(results, L, path):
    """fem2d_P2, p = 1.0: z and the Newton iterations of every level of the ladder."""
    a, b = results(f"solve{L}", "t256"), results(f"solve{L}", path)
    rows = json.loads(str(a["rows"]))
    assert any(_small(r) for r in rows), rows
    assert np.array_equal(a["rows"], b["rows"])
    assert np.isfinite(a["z"]).all()
    assert np.array_equal(a["its"], b["its"])
    assert np.array_equal(a["z"], b["z"])
