"""Hand-built fem1d levels for the column-split boundary product of the backward sweep's large-front launches
(csrc/mf_big_inv.hpp: mf_bwd_inv_split; csrc/mf_launch_plan.hpp: bwd_inv_split), in the manner of tests/solver_gate_cases.py and
built with its Builder: block arrows, nested block arrows (a separator coupled to a few columns of a clique above it) and
independent components side by side.  As there, the symbolic analysis decides the fronts, so every case pins the launch rows
and the fronts it gets, and with them the number S of workgroups per front that each large-front launch must be given.

What the cases are there for -- the smallest places the split kernel can go wrong:
  leaves_k33_k65  S = 2 and S = 3; k = 33 and k = 65 (the 4-column groups and the 32-column blocks both end ragged) beside
                  k = 100 and 115 in one launch of nine fronts: with S = 2 the second workgroup of the k = 33 front has no
                  column at all and that of the k = 65 front exactly one
  three           three fronts of different k in one launch, S = 4: k = 255 with m - k = 9, k = 63 and k = 18 (three of its
                  four workgroups without columns)
  thin8           m - k = 8 on every front of the launch: stays one workgroup per front
  root_mix        a front without boundary (the border row alone: one thread per column in the continuing workgroup) beside a
                  bordered one in a split launch, S = 4
  leaves9         five fronts, m - k = 9 on three of them, k = 200 / 197 / 226, S = 4
  cap16           one front, k = 1001, m - k = 9: S at its cap of 16

python backward_split_cases.py OUT.npz [CASE ...] is the worker process (the solver's switches are read once per process)."""
import functools
import os
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import gate_cases as G
import solver_gate_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADES = (0, 12)

# bwd_inv_split (csrc/mf_launch_plan.hpp), mirrored to pin S per launch; tests/csrc/bwd_split_check.cpp holds the C++ rule to
# the same triples (SPLIT_TRIPLES below)
def split_of(count, max_k, max_m):
    if count < 1 or max_m - max_k <= 8:
        return 1
    return max(1, min(16, 256 // count, (max_k + 63) // 64))


def _components(*comps, roots=()):
    """comps: (top, ks, s, nabove) -- a block arrow (ks, s) whose separator is coupled to the first nabove columns of a clique
    of `top` columns above it; roots: (ks, s) plain block arrows.  All side by side, uncoupled."""
    def build():
        b = S.Builder()
        for top, ks, s, nabove in comps:
            sep = b.cols(top)
            b.arrow(ks, s, above=sep[:nabove])
            b.clique(sep)
        for ks, s in roots:
            b.arrow(ks, s)
        return b
    return build


@dataclass
class Case:
    name: str
    build: object            # () -> Builder
    rows: list               # launch rows as shipped
    fronts: tuple            # (level, m, k, children, how many), sorted
    splits: dict             # tree level of a large-front launch on the inverse-based path -> S
    grades: tuple = GRADES


ROW_KEYS = ("level", "first", "count", "cls", "max_m", "max_k", "inv")      # the columns of a launch row that a case pins

CASES = [
    Case("leaves_k33_k65", S._arrows([33, 65, 255, 100, 100, 100, 100, 100, 100], 100),
         ((0, 0, 9, 0, 356, 115, 1), (1, 9, 1, 0, 241, 140, 1), (2, 10, 1, 128, 128, 127, 0), (3, 11, 1, 16, 1, 1, 0)),
         ((0, 134, 33, 0, 1), (0, 166, 65, 0, 1), (0, 201, 73, 0, 1), (0, 201, 100, 0, 5), (0, 356, 115, 0, 1), (1, 241, 140, 1, 1),
          (2, 128, 127, 9, 1), (3, 1, 1, 1, 1)),
         {0: 2, 1: 3}),
    Case("three", _components((100, [100] * 2, 33, 99), (100, [100] * 2, 65, 99), (40, [100] * 2, 255, 8)),
         ((0, 0, 8, 0, 356, 100, 1), (1, 8, 3, 0, 264, 255, 1), (2, 11, 3, 128, 102, 101, 0), (3, 14, 1, 16, 1, 1, 0)),
         ((0, 101, 1, 0, 1), (0, 134, 65, 0, 1), (0, 134, 82, 0, 1), (0, 134, 100, 0, 1), (0, 166, 100, 0, 2), (0, 356, 100, 0, 2),
          (1, 52, 18, 1, 1), (1, 165, 63, 2, 1), (1, 264, 255, 2, 1), (2, 41, 40, 1, 1), (2, 69, 68, 3, 1), (2, 102, 101, 2, 1),
          (3, 1, 1, 3, 1)),
         {0: 2, 1: 4}),
    Case("thin8", _components((40, [100] * 3, 255, 7), (40, [100] * 3, 250, 7)),
         ((0, 0, 6, 0, 356, 100, 1), (1, 6, 2, 0, 263, 255, 1), (2, 8, 2, 48, 41, 40, 0), (3, 10, 1, 16, 1, 1, 0)),
         ((0, 351, 100, 0, 3), (0, 356, 100, 0, 3), (1, 258, 250, 3, 1), (1, 263, 255, 3, 1), (2, 41, 40, 1, 2), (3, 1, 1, 2, 1)),
         {0: 2, 1: 1}),
    Case("root_mix", _components((40, [100] * 3, 255, 8), roots=[([100, 100, 100], 200)]),
         ((0, 0, 7, 0, 356, 100, 1), (1, 7, 2, 0, 272, 255, 1), (2, 9, 1, 32, 17, 16, 0), (3, 10, 1, 16, 1, 1, 0)),
         ((0, 41, 32, 0, 1), (0, 301, 100, 0, 3), (0, 356, 92, 0, 1), (0, 356, 100, 0, 2), (1, 201, 200, 3, 1), (1, 272, 255, 3, 1),
          (2, 17, 16, 2, 1), (3, 1, 1, 2, 1)),
         {0: 2, 1: 4}),
    Case("leaves9", S._arrows([255, 250, 200, 200, 200], 8),
         ((0, 0, 5, 0, 264, 226, 1), (1, 5, 1, 64, 62, 53, 0), (2, 6, 1, 48, 38, 37, 0), (3, 7, 1, 16, 1, 1, 0)),
         ((0, 209, 200, 0, 3), (0, 259, 197, 0, 1), (0, 264, 226, 0, 1), (1, 62, 53, 1, 1), (2, 38, 37, 5, 1), (3, 1, 1, 1, 1)),
         {0: 4}),
    Case("cap16", _components((40, [100] * 3, 1001, 8)),
         ((0, 0, 3, 0, 1102, 100, 1), (1, 3, 1, 0, 1010, 1001, 1), (2, 4, 1, 48, 41, 40, 0), (3, 5, 1, 16, 1, 1, 0)),
         ((0, 1102, 100, 0, 3), (1, 1010, 1001, 3, 1), (2, 41, 40, 1, 1), (3, 1, 1, 1, 1)),
         {0: 2, 1: 16}, grades=(0,)),
]
CASE = {c.name: c for c in CASES}
LEVEL = {c.name: l for l, c in enumerate(CASES)}

# (count, max_k, max_m, S) of every large-front launch above
SPLIT_TRIPLES = sorted({(r[2], r[5], r[4], c.splits[r[0]]) for c in CASES for r in c.rows if r[3] == 0 and r[6]})


def pinned(rows):
    """The pinned columns of launch rows (dicts, as DeviceProblem.solver_launches / solver_gate_cases.host_launches give them)."""
    return tuple(tuple(int(r[k]) for k in ROW_KEYS) for r in rows)


@functools.lru_cache(maxsize=None)
def built(name):
    b = CASE[name].build()
    assert len(b.elements) <= S.N_ELEMENTS and b.m <= 3000
    return b


@functools.lru_cache(maxsize=None)
def pattern(name):
    b = built(name)
    return S.pattern_of(b.elements, b.m)


def host_rows(name, **kw):
    b = built(name)
    return S.host_launches(*pattern(name), S.centroids(S.N_ELEMENTS, b.elements, b.m), **kw)


@functools.lru_cache(maxsize=None)
def problem():
    """One fem1d hierarchy: level l is CASES[l], the last level the true finest one (as solver_gate_cases.problem)."""
    return G.fem1d_problem(S.N_ELEMENTS, [S.level_matrices(S.N_ELEMENTS, built(c.name).elements, built(c.name).m) for c in CASES])


@functools.lru_cache(maxsize=None)
def system(name, grade):
    """(A, g): the recipe of solver_gate_cases.system on this module's patterns -- off-diagonals +-weight in [0.3, 0.95] with
    seeded signs, diagonal = absolute row sum + 1, scaled on both sides by 10^uniform(-grade/2, grade/2)."""
    indptr, indices = pattern(name)
    m = indptr.size - 1
    rng = np.random.default_rng(77000 + 1000 * LEVEL[name] + grade)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    sign = np.where(rng.random((m, 1)) < 0.5, -1.0, 1.0) * np.where(rng.random((1, m)) < 0.5, -1.0, 1.0)
    sgn = sign[lo, hi] * np.where((lo * 7919 + hi * 104729) % 3 == 0, -1.0, 1.0)
    v = np.where(rows == indices, 0.0, G.weight(3 * lo, hi) * sgn)
    core = sp.csr_matrix((v, indices, indptr), shape=(m, m))
    dia = np.asarray(abs(core).sum(axis=1)).ravel() + 1.0
    v = np.where(rows == indices, dia[rows], v)
    d = 10.0 ** rng.uniform(-grade / 2, grade / 2, m) if grade else np.ones(m)
    A = sp.csr_matrix((d[lo] * v * d[hi], indices.copy(), indptr.copy()), shape=(m, m))
    t = rng.uniform(0.5, 1.5, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    return A, A @ (t / d)


def run_cases(P, names, out):
    """Both solve paths of every (case, grade), twice on one factorization each time (the second sweep finds the arrival
    counters as the first left them), the relative residual of the first, and the launch rows."""
    import json
    for name in names:
        lev = LEVEL[name]
        for grade in CASE[name].grades:
            A, g = system(name, grade)
            key = f"{name}_g{grade}"
            P.set_hessian(lev, A.data)
            out[key + "_x"] = P.solve(lev, g)
            out[key + "_x_again"] = P.solve(lev, g)              # same factors: a second forward + backward sweep
            for rep in ("", "_again"):
                P.set_hessian(lev, A.data)
                xn, lam, status = P.solve_newton(lev, g, check=False)
                out[key + "_xn" + rep], out[key + "_lam" + rep] = xn, np.array([lam, float(status)])
            r = A @ out[key + "_x"] - g
            out[key + "_res"] = np.array(float(np.max(np.abs(r) / (abs(A) @ np.abs(out[key + "_x"]) + np.abs(g)))))
        ip, ix = P.hessian_pattern(lev)
        out[name + "_pattern_ok"] = np.array(np.array_equal(ip, pattern(name)[0]) and np.array_equal(ix, pattern(name)[1]))
        out[name + "_rows"] = np.array(json.dumps(P.solver_launches(lev)))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from mgb_amd.device import DeviceProblem, HipContext
    prob = problem()
    ctx = HipContext(0)
    P = DeviceProblem(ctx, prob.M[0], prob.Q)
    res = {}
    run_cases(P, sys.argv[2:] or [c.name for c in CASES], res)
    P.close()
    ctx.close()
    np.savez(sys.argv[1], **res)
