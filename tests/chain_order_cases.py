"""Cases and worker of tests/test_gpu_chain_order.py (the solver's switches are read once per process).

The large-front shapes the gate cases of tests/solver_gate_cases.py do not reach in one place, built with that module's Builder
as block arrows on a fem1d hierarchy of their own (level l is CASES[l]); every case carries the launch rows and fronts it must
get with MGBHIP_INV_MIN_N=0 (the inverse-based path for systems of any size), which the worker sets for this mode.

python chain_order_cases.py OUT.npz gates CASE [CASE ...] -- zero TAG [TAG ...]    gate cases and zero-pivot systems of
                                                                                  solver_gate_cases on its hierarchy, one process
python chain_order_cases.py OUT.npz new                                           the cases of this file
python chain_order_cases.py OUT.npz solve L [L ...]                               whole solves of fem2d_P2, p = 1.0"""
import functools
import json
import os
import sys
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import gate_cases as G
import solver_gate_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADES = (0, 12)
ENV = {"MGBHIP_INV_MIN_N": "0"}


@dataclass
class Case:
    name: str
    build: object           # () -> Builder
    rows: list              # launch rows under ENV
    fronts: tuple           # (level, m, k, children, how many), sorted
    what: str


def _arrows(ks, s):
    def build():
        b = S.Builder()
        b.arrow(ks, s)
        return b
    return build


# Row columns as in solver_gate_cases: level first count cls max_m max_k max_child | tiny wave inv iface packed |
# assembly (1 gather 2 columns) block0 (1 gather workgroup 2 mf_big_diag0 3 in step 0) backward | 0
CASES = [
    Case("mixed6", _arrows([33, 32, 31, 64, 65, 100], 100),
         S._rows((0, 0, 6, 0, 201, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
                 (1, 6, 2, 128, 110, 9, 1, 0, 0, 0, 0, 0, 0, 0, 2, 0),
                 (1, 8, 1, 0, 149, 48, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
                 (2, 9, 1, 128, 106, 105, 6, 0, 0, 0, 0, 0, 0, 0, 3, 0),
                 (3, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ((0, 132, 23, 0, 1), (0, 133, 23, 0, 1), (0, 134, 28, 0, 1), (0, 165, 16, 0, 1), (0, 166, 65, 0, 1), (0, 201, 100, 0, 1),
          (1, 109, 8, 1, 1), (1, 110, 9, 1, 1), (1, 149, 48, 1, 1), (2, 106, 105, 6, 1), (3, 1, 1, 1, 1)),
         "six childless fronts, m = 132 .. 201 and k = 16 (one block, no look-ahead) .. 100 (four blocks, the last of 4 columns), in "
         "ONE launch of < 24 fronts: column-tiled assembly, block 0 inside step 0, grids sized for m = 201 (the tile workgroups of "
         "the smaller fronts return at once); a gather launch of one front with one child, k = 48"),
    Case("one_child", _arrows([100] * 2, 28),
         S._rows((0, 0, 1, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
                 (1, 1, 1, 0, 129, 128, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
                 (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ((0, 129, 100, 0, 1), (1, 129, 128, 1, 1), (2, 1, 1, 1, 1)),
         "single-front launches: the gather's block-0 workgroup with 1 child, k = 128 = m - 1 (the last step's only tile is one row)"),
    Case("diag0_mixed", _arrows([100] * 12 + [60] * 13, 68),
         S._rows((0, 0, 25, 0, 169, 100, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0),
                 (1, 25, 6, 0, 157, 88, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
                 (2, 31, 1, 0, 145, 144, 25, 0, 0, 1, 0, 0, 2, 3, 0, 0),
                 (3, 32, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ((0, 129, 60, 0, 13), (0, 169, 12, 0, 2), (0, 169, 24, 0, 1), (0, 169, 28, 0, 1), (0, 169, 56, 0, 1), (0, 169, 62, 0, 1),
          (0, 169, 64, 0, 1), (0, 169, 100, 0, 5), (1, 105, 36, 1, 1), (1, 107, 38, 1, 1), (1, 113, 44, 1, 1), (1, 141, 72, 1, 1),
          (1, 157, 88, 1, 2), (2, 145, 144, 25, 1), (3, 1, 1, 1, 1)),
         "25 fronts of m = 129 and 169, k = 12 .. 100 (64 among them) in one launch with mf_big_diag0; six fronts of different m "
         "in one gather launch with the block-0 workgroup; a root with 25 children (column-tiled, block 0 in step 0)"),
]
CASE = {c.name: c for c in CASES}
LEVEL = {c.name: l for l, c in enumerate(CASES)}
N_ELEMENTS = 64


@functools.lru_cache(maxsize=None)
def built(name):
    b = CASE[name].build()
    assert len(b.elements) <= N_ELEMENTS and b.m <= 3000
    return b


@functools.lru_cache(maxsize=None)
def pattern(name):
    b = built(name)
    return S.pattern_of(b.elements, b.m)


def host_rows(name, **kw):
    """Launch rows of a case from the CPU build of the classification (oracle/csrc/mf_host.cpp), under ENV."""
    b = built(name)
    return S.host_launches(*pattern(name), S.centroids(N_ELEMENTS, b.elements, b.m), env=ENV, **kw)


@functools.lru_cache(maxsize=None)
def problem():
    return G.fem1d_problem(N_ELEMENTS, [S.level_matrices(N_ELEMENTS, built(c.name).elements, built(c.name).m) for c in CASES])


@functools.lru_cache(maxsize=None)
def system(name, grade):
    """(A, g) as solver_gate_cases.system builds them: off-diagonals +-weight with seeded signs, diagonal = absolute row sum + 1,
    scaled on both sides by 10^(+-grade/2); g = A x_true with x_true = D^-1 t, |t| in [0.5, 1.5]."""
    indptr, indices = pattern(name)
    m = indptr.size - 1
    rng = np.random.default_rng(7000 + 10 * LEVEL[name] + grade)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    sign = np.where(rng.random((m, 1)) < 0.5, -1.0, 1.0) * np.where(rng.random((1, m)) < 0.5, -1.0, 1.0)
    v = np.where(rows == indices, 0.0, G.weight(3 * lo, hi) * sign[lo, hi] * np.where((lo * 7919 + hi * 104729) % 3 == 0, -1.0, 1.0))
    core = sp.csr_matrix((v, indices, indptr), shape=(m, m))
    dia = np.asarray(abs(core).sum(axis=1)).ravel() + 1.0
    v = np.where(rows == indices, dia[rows], v)
    d = 10.0 ** rng.uniform(-grade / 2, grade / 2, m) if grade else np.ones(m)
    A = sp.csr_matrix((d[lo] * v * d[hi], indices.copy(), indptr.copy()), shape=(m, m))
    t = rng.uniform(0.5, 1.5, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    return A, A @ (t / d)


def run_new(P, out):
    """Both solve paths of every (case, grade), twice; the launch rows after the first solve."""
    for c in CASES:
        lev = LEVEL[c.name]
        for grade in GRADES:
            A, g = system(c.name, grade)
            key = f"{c.name}_g{grade}"
            for rep in ("", "_again"):
                P.set_hessian(lev, A.data)
                out[key + "_x" + rep] = P.solve(lev, g)
                P.set_hessian(lev, A.data)
                xn, lam, status = P.solve_newton(lev, g, check=False)
                out[key + "_xn" + rep], out[key + "_lam" + rep] = xn, np.array([lam, float(status)])
        ip, ix = P.hessian_pattern(lev)
        out[c.name + "_pattern_ok"] = np.array(np.array_equal(ip, pattern(c.name)[0]) and np.array_equal(ix, pattern(c.name)[1]))
        out[c.name + "_rows"] = np.array(json.dumps(P.solver_launches(lev)))


def run_solves(Ls, out):
    import mgb_amd as m
    from mgb_amd.device import DeviceMGBProblem
    from mgb_amd.solve import mgb_driver
    for L in Ls:
        prob = m.assemble(m.amg(m.subdivide(m.fem2d_P2(), L), prolongator=m.amg_ruge_stuben()), p=1.0)
        D = DeviceMGBProblem(prob, device_id=0)
        SOL = mgb_driver(D)
        fine = len(D.main.level_sizes) - 1
        out[f"L{L}_z"], out[f"L{L}_its"] = SOL["z"], np.asarray(SOL["SOL_main"]["its"])
        out[f"L{L}_rows"] = np.array(json.dumps(D.main.solver_launches(fine)))
        D.close()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    mode, args = sys.argv[2], sys.argv[3:]
    res = {}
    if mode == "solve":
        run_solves([int(a) for a in args], res)
    else:
        if mode == "new":
            os.environ.update(ENV)
        from mgb_amd.device import DeviceProblem, HipContext
        prob = problem() if mode == "new" else S.problem()
        ctx = HipContext(0)
        P = DeviceProblem(ctx, prob.M[0], prob.Q)
        if mode == "new":
            run_new(P, res)
        else:
            cut = args.index("--")
            S.run_cases(P, args[:cut], res)
            assert args[cut + 1] == "zero"
            S.run_zero_pivots(P, args[cut + 2:], res)
        P.close()
        ctx.close()
    np.savez(sys.argv[1], **res)
