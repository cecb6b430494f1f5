"""A carried factorization (`factor(level, g)` + `trisolve_carried`) leaves out the two launches of the 1 x 1 border front
(csrc/mf_numeric.hip: MfSolver::skips_border): its pivot -1 - lambda^2 is read by nobody, and its backward launch only stores
x[n] = 1, which the kernel that writes the border column now stores instead.  MGBHIP_BORDER_LAUNCHES=1 restores both launches.
No floating-point operation changes, so every comparison is bitwise.  Worker processes (the switch is read once per process):
tests/border_skip_worker.py on every level of a fem2d_P2 hierarchy and on the zero-pivot matrices of
tests/solver_gate_cases.py, that module's own worker on its gate cases, and one whole solve.

A generic solve() after a carried factorization cannot be requested through the C interface (mgbhip_solve factors first); the
state record refuses it (csrc/hessian_state.hpp: may_solve, held to its model by tests/test_hessian_state_host.py) and
MfSolver::solve itself refuses factors without a border pivot."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_gate_cases as S

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
PATHS = {"skip": {}, "launch": {"MGBHIP_BORDER_LAUNCHES": "1"}}
SWITCHES = ("MGBHIP_BORDER_LAUNCHES", "MGBHIP_SMALL_THREADS")

# The smallest refinement of fem2d_P2 whose ladder has a tiny (the coarsest levels: one front), a wave, an LDS and a large root
# front under the border: the fine level's root separator has 255 pivots at L = 7 (127 at L = 6: still an LDS front).
LADDER_L = 7
# gate cases by the root front under the border (the launch row before the last); a tiny root needs a system of one front,
# which only the ladder has
GATE_CASES = ["tiny", "wave_c8", "lds128", "merge255", "big129", "n1024", "ch8", "leaf_lds"]
REJECT_TAGS = ["tiny_last", "wave", "lds128_col8", "block0_step0", "block0_gather"]


def _worker(script, args, env, timeout=600):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, os.path.join(HERE, script), *args], capture_output=True, text=True, timeout=timeout,
                       env=dict(e, **env))
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """(kind, path) -> arrays of one worker: computed once, shared by the tests, never changed."""
    d = tmp_path_factory.mktemp("border_skip")
    cache = {}

    def get(kind, path):
        if (kind, path) not in cache:
            out = str(d / f"{kind}_{path}.npz")
            if kind == "ladder":
                _worker("border_skip_worker.py", [out, "ladder", str(LADDER_L)], PATHS[path])
            elif kind == "reject":
                _worker("border_skip_worker.py", [out, "reject"] + REJECT_TAGS, dict(PATHS[path], MGBHIP_NO_LU_FALLBACK="1"))
            elif kind == "gates":
                _worker("solver_gate_cases.py", [out] + GATE_CASES, PATHS[path])
            elif kind == "zero":
                _worker("solver_gate_cases.py", [out, "zero"] + REJECT_TAGS, PATHS[path])
            else:
                _worker("gather_maps_worker.py", [out, "6"], PATHS[path])
            cache[kind, path] = dict(np.load(out))
        return cache[kind, path]
    return get


def root_kind(rows):
    """Kernel family of the last real tree level (the fronts under the border front)."""
    assert rows[-1]["count"] == 1 and rows[-1]["max_m"] == 1 and rows[-1]["max_k"] == 1, rows[-1]
    r = [x for x in rows if x["level"] == rows[-1]["level"] - 1][-1]
    return "tiny" if r["tiny"] else ("wave" if r["wave"] else ("lds" if r["cls"] else "large"))


def test_gate_cases_cover_the_root_kinds():
    kinds = {root_kind(S.CASE[name].rows) for name in GATE_CASES}
    assert kinds == {"wave", "lds", "large"}, kinds


def test_ladder_directions_are_bitwise_the_same_without_the_border_launches(results):
    a, b = results("ladder", "skip"), results("ladder", "launch")
    nlev = int(a["levels"])
    assert nlev == int(b["levels"]) and nlev >= 3
    kinds = set()
    for J in range(nlev):
        assert np.array_equal(a[f"l{J}_rows"], b[f"l{J}_rows"])
        kinds.add(root_kind(json.loads(str(a[f"l{J}_rows"]))))
        for key in ("xa", "lama", "xb", "lamb", "xg", "xc", "lamc"):         # lam*: lambda^2, status word, condensed leaves
            assert np.array_equal(a[f"l{J}_{key}"], b[f"l{J}_{key}"], equal_nan=True), (J, key)
        assert np.isfinite(a[f"l{J}_xa"]).all() and float(a[f"l{J}_lama"][1]) == 0.0, J
        # the second factorization and sweep, and the one after a generic solve, repeat the first where the leaves were formed
        # the same way (a level with condensed leaves forms them in the element kernel from the second direction on)
        if float(a[f"l{J}_lama"][2]) == float(a[f"l{J}_lamb"][2]):
            assert np.array_equal(a[f"l{J}_xa"], a[f"l{J}_xb"]), J
        assert np.array_equal(a[f"l{J}_xb"], a[f"l{J}_xc"]), J
    print("root fronts under the border on the ladder:", sorted(kinds))
    assert kinds == {"tiny", "wave", "lds", "large"}, kinds


@pytest.mark.parametrize("name", GATE_CASES)
def test_gate_case_is_bitwise_the_same_without_the_border_launches(results, name):
    """Both paths of the worker: the generic factor + solve (identity border: it keeps the border front's launches under
    either setting, and needs its pivot) and the carried one, each twice."""
    a, b = results("gates", "skip"), results("gates", "launch")
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


@pytest.mark.parametrize("tag", REJECT_TAGS)
def test_rejected_solve_then_a_regular_matrix(results, tag):
    """A zero pivot inside a tiny, a wave, an LDS and a large front: the carried path reports it alike (no LU fallback here),
    and the regular matrix factored next on the same level gives the same bits, twice, as does a generic solve after it."""
    from mgb_amd import device as dev
    a, b = results("reject", "skip"), results("reject", "launch")
    for r in (a, b):
        assert float(r[tag + "_zero"][1]) == dev.ERR_NOT_SPD, (tag, r[tag + "_zero"])
        assert float(r[tag + "_lam"][1]) == 0.0 and np.isfinite(r[tag + "_x"]).all(), tag
        assert np.array_equal(r[tag + "_x"], r[tag + "_x_again"]) and np.array_equal(r[tag + "_lam"], r[tag + "_lam_again"]), tag
    assert np.array_equal(a[tag + "_rows"], b[tag + "_rows"])
    for key in ("_zero_x", "_zero", "_x", "_lam", "_x_again", "_lam_again", "_xg"):
        assert np.array_equal(a[tag + key], b[tag + key], equal_nan=True), (tag, key)


@pytest.mark.parametrize("tag", REJECT_TAGS)
def test_zero_pivot_verdict_with_the_lu_fallback(results, tag):
    """The same matrices with the pivoted-LU fallback in place: status and solution of both solve paths agree."""
    a, b = results("zero", "skip"), results("zero", "launch")
    for key in ("_status", "_statusn", "_x", "_xn", "_lam"):
        assert np.array_equal(a[tag + key], b[tag + key], equal_nan=True), (tag, key)


def test_whole_solve_is_bitwise_the_same_without_the_border_launches(results):
    a, b = results("solve", "skip"), results("solve", "launch")
    assert np.isfinite(a["z"]).all()
    assert np.array_equal(a["rows"], b["rows"])
    assert np.array_equal(a["its"], b["its"])
    assert np.array_equal(a["z"], b["z"])
