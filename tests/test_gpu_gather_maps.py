"""The static gather maps of mf_big_gather (csrc/mf_launch_plan.hpp: build_gather_maps) against the kernel that rebuilds its
index tables in LDS at every launch (MGBHIP_GATHER_LDS_MAPS=1), and the wider column tiles of launches with many fronts
(big_gather_ct; forced here with MGBHIP_GATHER_CT, since only levels of several hundred workgroups choose them) against the
8-column ones.  The arithmetic is the same -- children in child order, one register sum per destination entry, the matrix
entries added after it -- so every comparison is bitwise.  Worker processes: the switches are read once per process; one
worker per path runs all the gate cases."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_gate_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"maps": {}, "lds": {"MGBHIP_GATHER_LDS_MAPS": "1"}, "ct16": {"MGBHIP_GATHER_CT": "16"}, "ct32": {"MGBHIP_GATHER_CT": "32"}}
OTHERS = [p for p in PATHS if p != "maps"]
SWITCHES = ("MGBHIP_GATHER_LDS_MAPS", "MGBHIP_GATHER_CT")

# every gate case with a gather launch: 1 child at m = 129 (big129), 7 and 8 children (gather7, ch8), the 8 x 1280 table at the
# kernel's cap with k = 1279, m - k = 1 (edge10240), tiny square leaves under a large-front parent (leaf_big_subst), mixed k ...
GATHER_CASES = [c.name for c in S.CASES if any(r["assembly"] == "gather" for r in c.rows)]


def _worker(script, args, env, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(e, **env))
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """path -> arrays of one worker: computed once, shared by the tests, never changed."""
    d = tmp_path_factory.mktemp("gather_maps")
    cache = {}

    def get(kind, path):
        if (kind, path) not in cache:
            out = str(d / f"{kind}_{path}.npz")
            if kind == "gates":
                _worker("solver_gate_cases.py", [out] + GATHER_CASES, PATHS[path])
            elif kind == "solve":
                _worker("gather_maps_worker.py", [out, "7"], PATHS[path])
            else:               # zero pivot in the gather workgroup, with (zero) and without (zero_nofb) the pivoted-LU fallback
                env = dict(PATHS[path], **({"MGBHIP_NO_LU_FALLBACK": "1"} if kind == "zero_nofb" else {}))
                _worker("solver_gate_cases.py", [out, "zero", "block0_gather"], env)
            cache[kind, path] = dict(np.load(out))
        return cache[kind, path]
    return get


def test_the_gather_cases_are_the_ones_the_maps_were_built_for():
    assert {"big129", "gather7", "ch8", "edge10240", "leaf_big_subst"} <= set(GATHER_CASES)


@pytest.mark.parametrize("name", GATHER_CASES)
def test_gate_case_has_its_rows_and_is_reproducible(results, name):
    a = results("gates", "maps")
    assert bool(a[name + "_pattern_ok"])
    assert json.loads(str(a[name + "_rows"])) == S.CASE[name].rows, name
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam"):
            key = f"{name}_g{grade}{suffix}"
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], a[key + "_again"]), key


@pytest.mark.parametrize("path", OTHERS)
@pytest.mark.parametrize("name", GATHER_CASES)
def test_gate_case_is_bitwise_the_same_on_every_path(results, name, path):
    a, b = results("gates", "maps"), results("gates", path)
    assert bool(b[name + "_pattern_ok"])
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam"):
            key = f"{name}_g{grade}{suffix}"
            assert np.array_equal(a[key], b[key]), (key, path)


def test_zero_pivot_in_the_gather_workgroup_is_reported_alike(results):
    """ZERO_PIVOTS tag block0_gather: the diagonal-block workgroup reads the maps.  Without the LU fallback both paths flag
    the pivot; with it both return the same solution."""
    from mgb_amd import device as dev
    for path in ("maps", "lds"):
        r = results("zero_nofb", path)
        for key in ("block0_gather_status", "block0_gather_statusn"):
            assert float(r[key]) == dev.ERR_NOT_SPD, (path, key, float(r[key]))
    a, b = results("zero", "maps"), results("zero", "lds")
    for key in ("block0_gather_status", "block0_gather_statusn"):
        assert float(a[key]) == float(b[key]) == 0.0, key
    for key in ("block0_gather_x", "block0_gather_xn", "block0_gather_lam"):
        assert np.array_equal(a[key], b[key]), key


@pytest.mark.parametrize("path", OTHERS)
def test_whole_solve_is_bitwise_the_same_on_every_path(results, path):
    """fem2d_P2, p = 1.0, L = 7: the smallest refinement whose fine level has large fronts (root separator k = 255)."""
    a, b = results("solve", "maps"), results("solve", path)
    rows = json.loads(str(a["rows"]))
    assert any(r["assembly"] == "gather" for r in rows), rows
    assert any(r["block0"] == "gather" for r in rows), rows
    assert np.array_equal(a["rows"], b["rows"])
    assert np.isfinite(a["z"]).all()
    assert np.array_equal(a["its"], b["its"])
    assert np.array_equal(a["z"], b["z"])
