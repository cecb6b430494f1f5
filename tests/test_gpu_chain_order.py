"""The chain-first grids of mf_big_step and mf_big_gather (csrc/mf_block_roles.hpp: every front's chain workgroup -- the
look-ahead workgroup of a pivot step, the block-0 workgroup of the gathering assembly -- ahead of every tile in dispatch order)
against the layout before them (MGBHIP_CHAIN_ORDER=legacy: the chain workgroup last in its front's row of the grid), and, on
the cases of tests/chain_order_cases.py, each kernel switched alone (`step`, `gather`).  The layout decides which workgroup
index does which role and nothing else -- no workgroup of these launches reads what another one of the same launch writes --
so every comparison is bitwise.  Nothing here asserts a timing or a dispatch order.  Worker processes
(tests/chain_order_cases.py): the switch is read once per process.

The library has no read-back of the frontal arena; the factors are compared through what they determine, the generic solve
(forward and backward sweep over every factor entry) and the carried one (the factorization's own forward substitution: the
Newton direction and lambda^2), with the status word, on two gradings and twice each.

Shapes, by the pinned plans of the cases (checked below):
  k = 31, 32 (no look-ahead block), 33 (a look-ahead block of one column), 65      rule1_accept
  k = 64                                                                           k1_rule1, diag0_mixed
  one launch holding fronts of different m                                         rule1_accept (m = 76 .. 129), mixed6, diag0_mixed
  a launch of >= 24 fronts (mf_big_diag0)                                          c24, d24, diag0_mixed
  < 24 fronts without the gathering assembly (block 0 inside step 0)               n1024, k1_inv, leaf_big_inv, mixed6
  the gather's block-0 workgroup with 1 / 7 / 8 children                           one_child, rule1_accept / mixed_inv, gather7 / ch8
  a step whose only tile is a single row (m - j1 = 1)                              every root front (k = m - 1)
A step with NO tile (m = j1, where the chain workgroup itself writes M_j home) does not occur through the library: every
front of a DeviceProblem carries the border row, so m >= k + 1; that branch of the kernel is the same text in both layouts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import chain_order_cases as C
import solver_gate_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"first": {}, "legacy": {"MGBHIP_CHAIN_ORDER": "legacy"}, "step": {"MGBHIP_CHAIN_ORDER": "step"},
         "gather": {"MGBHIP_CHAIN_ORDER": "gather"}}
OTHERS = [p for p in PATHS if p != "legacy"]
SWITCHES = ("MGBHIP_CHAIN_ORDER", "MGBHIP_INV_MIN_N", "MGBHIP_NO_LU_FALLBACK")

GATE_CASES = ["big129", "mixed_inv", "k1_inv", "leaf_big_inv", "rule1_accept", "k1_rule1", "n1024", "c24", "d24", "gather7", "ch8"]
ZERO_TAGS = ["block0_step0", "block0_diag0", "block0_gather", "pivot32", "ragged_last"]       # the large-front placements
NEW_CASES = [c.name for c in C.CASES]


def _worker(args, env, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(HERE, "chain_order_cases.py"), *args], capture_output=True, text=True,
                       timeout=timeout, env=dict(e, **env))
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """(kind, path) -> arrays of one worker: computed once, shared by the tests, never changed."""
    d = tmp_path_factory.mktemp("chain_order")
    cache = {}

    def get(kind, path):
        if (kind, path) not in cache:
            out = str(d / f"{kind}_{path}.npz")
            if kind == "gates":
                _worker([out, "gates", *GATE_CASES, "--", "zero", *ZERO_TAGS], PATHS[path])
            elif kind == "zero_nofb":
                _worker([out, "gates", "--", "zero", *ZERO_TAGS], dict(PATHS[path], MGBHIP_NO_LU_FALLBACK="1"))
            elif kind == "new":
                _worker([out, "new"], PATHS[path])
            else:
                _worker([out, "solve", "5", "6"], PATHS[path])
            cache[kind, path] = dict(np.load(out))
        return cache[kind, path]
    return get


def test_the_cases_hold_the_shapes():
    fronts = {name: S.CASE[name].fronts for name in GATE_CASES}
    fronts.update({c.name: c.fronts for c in C.CASES})
    rows = {name: S.CASE[name].rows for name in GATE_CASES}
    rows.update({c.name: c.rows for c in C.CASES})

    def big(name):          # the large-front launches on the inverse-based path
        return [r for r in rows[name] if r["cls"] == 0 and r["inv"]]

    def ks(name, level=0):
        return {k for (lev, m, k, nch, cnt) in fronts[name] if lev == level and m > 1}
    assert {31, 32, 33, 65} <= ks("rule1_accept") and big("rule1_accept")[0]["count"] == 16      # folded into the large-front launch
    assert 64 in ks("k1_rule1") and 64 in ks("diag0_mixed") and 1 in ks("k1_inv")
    for name in ("rule1_accept", "mixed6", "diag0_mixed"):                                        # different m in one launch
        ms = {m for (lev, m, k, nch, cnt) in fronts[name] if lev == 0}
        assert big(name)[0]["level"] == 0 and big(name)[0]["count"] == sum(c for (lev, *_, c) in fronts[name] if lev == 0)
        assert len({(m - 32 + 63) // 64 for m in ms}) > 1, name                                   # and different tile counts at step 0
    for name in ("c24", "d24", "diag0_mixed"):
        assert big(name)[0]["count"] >= 24 and big(name)[0]["block0"] == "diag0", name
    for name in ("n1024", "k1_inv", "leaf_big_inv", "mixed6"):
        assert any(r["count"] < 24 and r["assembly"] == "columns" and r["block0"] == "step0" for r in big(name)), name
    for name, nch in (("one_child", 1), ("rule1_accept", 1), ("mixed_inv", 7), ("gather7", 7), ("ch8", 8)):
        assert any(r["assembly"] == "gather" and r["block0"] == "gather" and r["max_child"] == nch for r in big(name)), name
    assert any(r["assembly"] == "gather" and r["block0"] == "gather" and r["count"] == 6 for r in big("diag0_mixed"))
    assert all(any(k == m - 1 and m > 129 for (lev, m, k, nch, cnt) in fronts[name]) for name in ("k1_inv", "rule1_accept", "diag0_mixed"))
    assert not any(m == k and m > 1 for f in fronts.values() for (lev, m, k, nch, cnt) in f)      # no step without a tile


@pytest.mark.parametrize("name", NEW_CASES)
def test_new_case_has_its_rows_and_is_reproducible(results, name):
    a = results("new", "legacy")
    assert bool(a[name + "_pattern_ok"])
    assert json.loads(str(a[name + "_rows"])) == C.CASE[name].rows, name
    for grade in C.GRADES:
        for suffix in ("_x", "_xn", "_lam"):
            key = f"{name}_g{grade}{suffix}"
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], a[key + "_again"]), key
        assert float(a[f"{name}_g{grade}_lam"][1]) == 0.0


@pytest.mark.parametrize("path", OTHERS)
@pytest.mark.parametrize("name", NEW_CASES)
def test_new_case_is_bitwise_the_same_in_every_layout(results, name, path):
    a, b = results("new", "legacy"), results("new", path)
    assert bool(b[name + "_pattern_ok"])
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in C.GRADES:
        for suffix in ("_x", "_xn", "_lam", "_x_again", "_xn_again", "_lam_again"):
            key = f"{name}_g{grade}{suffix}"
            assert np.array_equal(a[key], b[key]), (key, path)


@pytest.mark.parametrize("name", GATE_CASES)
def test_gate_case_has_its_rows_in_the_legacy_layout(results, name):
    a = results("gates", "legacy")
    assert bool(a[name + "_pattern_ok"])
    assert json.loads(str(a[name + "_rows"])) == S.CASE[name].rows, name


@pytest.mark.parametrize("path", ["first"])
@pytest.mark.parametrize("name", GATE_CASES)
def test_gate_case_is_bitwise_the_same_in_every_layout(results, name, path):
    a, b = results("gates", "legacy"), results("gates", path)
    assert bool(b[name + "_pattern_ok"])
    assert np.array_equal(a[name + "_rows"], b[name + "_rows"])
    for grade in S.CASE[name].grades:
        for suffix in ("_x", "_xn", "_lam", "_x_again", "_xn_again", "_lam_again"):
            key = f"{name}_g{grade}{suffix}"
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], b[key]), (key, path)


@pytest.mark.parametrize("path", ["first"])
def test_zero_pivots_are_reported_and_repaired_alike(results, path):
    """Without the LU fallback every layout flags the pivot, with the same (possibly non-finite) vectors; with it every layout
    returns the same solution."""
    from mgb_amd import device as dev
    a, b = results("zero_nofb", "legacy"), results("zero_nofb", path)
    for tag in ZERO_TAGS:
        for key in (tag + "_status", tag + "_statusn"):
            assert float(a[key]) == float(b[key]) == dev.ERR_NOT_SPD, (path, key)
        for key in (tag + "_x", tag + "_xn", tag + "_lam"):
            assert np.array_equal(a[key], b[key], equal_nan=True), (path, key)
    a, b = results("gates", "legacy"), results("gates", path)
    for tag in ZERO_TAGS:
        for key in (tag + "_status", tag + "_statusn"):
            assert float(a[key]) == float(b[key]) == 0.0, (path, key)
        for key in (tag + "_x", tag + "_xn", tag + "_lam"):
            assert np.isfinite(a[key]).all() and np.array_equal(a[key], b[key]), (path, key)


@pytest.mark.parametrize("path", ["first"])
@pytest.mark.parametrize("L", [5, 6])
def test_whole_solve_is_bitwise_the_same(results, L, path):
    """fem2d_P2, p = 1.0: z and the Newton iterations of every level of the ladder."""
    a, b = results("solves", "legacy"), results("solves", path)
    assert np.array_equal(a[f"L{L}_rows"], b[f"L{L}_rows"])
    assert np.isfinite(a[f"L{L}_z"]).all()
    assert np.array_equal(a[f"L{L}_its"], b[f"L{L}_its"])
    assert np.array_equal(a[f"L{L}_z"], b[f"L{L}_z"])
