"""The column-split boundary product of the backward sweep's large-front launches (csrc/mf_big_inv.hpp: mf_bwd_inv_split, S
workgroups per front, the last to arrive runs the block recurrence) against one workgroup per front (MGBHIP_BWD_SPLIT=0:
mf_bwd_inv for every launch).  A pivot column's boundary sum is formed by one wave with the unsplit kernel's loop and
reductions, whichever workgroup owns it, so every comparison is bitwise.  Worker processes (the switch is read once per
process): one per path and kind -- the gate cases of tests/solver_gate_cases.py that have a large-front launch on the
inverse-based path, the cases of tests/backward_split_cases.py built for the split kernel, and one whole solve."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import backward_split_cases as B
import solver_gate_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"split": {}, "one": {"MGBHIP_BWD_SPLIT": "0"}}
SWITCHES = ("MGBHIP_BWD_SPLIT",)

# gate cases whose backward sweep reaches mf_bwd_inv: a large-front launch (cls 0) on the inverse-based path
GATE_CASES = [c.name for c in S.CASES if any(r["cls"] == 0 and r["inv"] for r in c.rows)]
SPLIT_CASES = [c.name for c in B.CASES]
# Componentwise backward error of a solve, as tests/solver_gate_cases.py bounds it for every kernel family (ETA_MAX = 4e-12).  Here
# the residual is formed in double precision: a row of at most 1102 entries adds at most 1103 * 2^-53 = 1.3e-13 to the quotient.
ETA_MAX = S.ETA_MAX + 1.3e-13


def _worker(script, args, env, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(e, **env))
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """(kind, path) -> arrays of one worker: computed once, shared by the tests, never changed."""
    d = tmp_path_factory.mktemp("backward_launches")
    cache = {}

    def get(kind, path):
        if (kind, path) not in cache:
            out = str(d / f"{kind}_{path}.npz")
            if kind == "gates":
                _worker("solver_gate_cases.py", [out] + GATE_CASES, PATHS[path])
            elif kind == "split":
                _worker("backward_split_cases.py", [out] + SPLIT_CASES, PATHS[path])
            else:               # solve7, solve8
                _worker("gather_maps_worker.py", [out, kind[len("solve"):]], PATHS[path])
            cache[kind, path] = dict(np.load(out))
        return cache[kind, path]
    return get


def test_some_gate_cases_have_split_launches():
    split = {c.name for c in S.CASES for r in c.rows
             if r["cls"] == 0 and r["inv"] and B.split_of(r["count"], r["max_k"], r["max_m"]) > 1}
    assert {"rule1_accept", "n1024", "k1_inv", "edge10240"} <= split <= set(GATE_CASES), split


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_case_has_its_rows_solves_and_repeats(results, name):
    a = results("split", "split")
    assert bool(a[name + "_pattern_ok"])
    assert B.pinned(json.loads(str(a[name + "_rows"]))) == B.CASE[name].rows, name
    for grade in B.CASE[name].grades:
        key = f"{name}_g{grade}"
        for suffix in ("_x", "_xn", "_lam"):
            assert np.isfinite(a[key + suffix]).all(), key
            assert np.array_equal(a[key + suffix], a[key + suffix + "_again"]), key + suffix     # the counters were reset
        print(key, "eta", float(a[key + "_res"]))
        assert float(a[key + "_res"]) <= ETA_MAX, (key, float(a[key + "_res"]))
        assert float(a[key + "_lam"][1]) == 0.0


@pytest.mark.parametrize("name", SPLIT_CASES)
def test_split_case_is_bitwise_the_same_with_one_workgroup_per_front(results, name):
    a, b = results("split", "split"), results("split", "one")
    assert bool(b[name + "_pattern_ok"])
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in B.CASE[name].grades:
        for suffix in ("_x", "_x_again", "_xn", "_xn_again", "_lam", "_lam_again"):
            key = f"{name}_g{grade}{suffix}"
            assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("name", GATE_CASES)
def test_gate_case_is_bitwise_the_same_with_one_workgroup_per_front(results, name):
    a, b = results("gates", "split"), results("gates", "one")
    assert bool(a[name + "_pattern_ok"]) and bool(b[name + "_pattern_ok"])
    assert json.loads(str(a[name + "_rows"])) == S.CASE[name].rows, name
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam"):
            key = f"{name}_g{grade}{suffix}"
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], a[key + "_again"]), key
            assert np.array_equal(a[key], b[key]), key
            assert np.array_equal(a[key + "_again"], b[key + "_again"]), key


@pytest.mark.parametrize("L", [7, 8])
def test_whole_solve_is_bitwise_the_same_with_one_workgroup_per_front(results, L):
    """fem2d_P2, p = 1.0.  L = 7: the large fronts of the fine level have at most 63 pivots (measured: 4 / 8 / 4 / 2 fronts of
    k <= 31 / 31 / 63 / 63), so every launch keeps one workgroup per front and the switch must change nothing.  L = 8 is the
    smallest refinement with split launches in a whole solve (k = 127 on the levels of 2 and 4 fronts: S = 2)."""
    a, b = results(f"solve{L}", "split"), results(f"solve{L}", "one")
    rows = json.loads(str(a["rows"]))
    big = [(r["level"], r["count"], r["max_k"], r["max_m"], int(r["inv"])) for r in rows if r["cls"] == 0]
    print("large-front launches (level, count, max_k, max_m, inv):", big)
    splits = [B.split_of(count, max_k, max_m) for _, count, max_k, max_m, inv in big if inv]
    assert splits and min(splits) == 1, big
    if L == 8:
        assert max(splits) > 1, big
    assert np.array_equal(a["rows"], b["rows"])
    assert np.isfinite(a["z"]).all()
    assert np.array_equal(a["its"], b["its"])
    assert np.array_equal(a["z"], b["z"])
