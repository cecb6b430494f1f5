"""Hand-built fem1d levels that put the shape-gated kernels of the sparse LDL' (csrc/mf_launch_plan.hpp: classify_launches, the
merge rules, the launchers' predicates; DESIGN.md "Solver shape gates") on both sides of their gates, with an exact residual.

One fem1d hierarchy (tests/gate_cases.fem1d_problem) carries every case as a synthetic level R = blockdiag(U, S).  Two columns
of a level are coupled in its Hessian iff their supports share an element, so a list of column sets -- one element per set --
gives the level any pattern that is a union of cliques.  The building block is a block arrow: q cliques of k_i unknowns, each
coupled to a shared separator clique of s unknowns; block arrows nest.  The symbolic analysis (peeling, dissection,
amalgamation) decides the fronts, not the case author: every case carries the literal launch rows it must get
(DeviceProblem.solver_launches).  tests/test_solver_gate_cases.py checks them against the CPU build of the same classification
(oracle/csrc/mf_host.cpp: mf_host_launches), tests/test_gpu_solver_gates.py against the device.

Matrices go through set_hessian on the case's pattern: off-diagonals of magnitude gate_cases.weight in [0.3, 0.95] with seeded
signs, each diagonal entry its row's absolute sum + 1, scaled on both sides by 10^(+-grade/2) as solver_cases.graded_spd does;
g = A x_true with x_true = D^-1 t, |t| in [0.5, 1.5] (see `system`).  The checked quantity is the componentwise backward error (Oettli-Prager)
eta = max_i |A x - g|_i / (|A| |x| + |g|)_i with the residual formed exactly (gate_cases.exact_sum) and rounded once."""
import ctypes as C
import functools
import os
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import gate_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRADES = (0, 12)
ROW = 16
ETA_MAX = 4e-12            # tests/test_gpu_solver.py: ETA_MAX (a GPU module; tests/test_gpu_solver_gates.py asserts the two are equal)


# ---------------------------------------------------------------------------------------------------------------------
# patterns: column sets -> (U, S), the level Hessian's pattern, the ordering hint
# ---------------------------------------------------------------------------------------------------------------------

class Builder:
    """Collects cliques of columns (one element each).  Column 0 is the level's single u column; the others are slack columns."""

    def __init__(self):
        self.m = 0
        self.elements = []

    def cols(self, count):
        out = list(range(self.m, self.m + count))
        self.m += count
        return out

    def clique(self, *groups):
        self.elements.append(sorted(c for g in groups for c in g))

    def arrow(self, ks, s, above=()):
        """q cliques of ks[i] columns under a separator of s columns (itself coupled to `above`).  Returns the separator."""
        sep = self.cols(s)
        for k in ks:
            self.clique(self.cols(k), sep)
        if above or not ks:
            self.clique(sep, above)
        return sep


def level_matrices(N, elements, m):
    """(U, S) of a level with m columns whose element e (both broken nodes) carries the columns elements[e]."""
    assert len(elements) <= N and m >= 2
    ru, rs, cs = [], [], []
    for e, cols in enumerate(elements):
        for node in (2 * e, 2 * e + 1):
            for c in cols:
                if c == 0:
                    ru.append(node)
                else:
                    rs.append(node); cs.append(c - 1)
    ru, rs, cs = np.asarray(ru, dtype=np.int64), np.asarray(rs, dtype=np.int64), np.asarray(cs, dtype=np.int64)
    xi = ((ru + 1) // 2) / N
    U = sp.csr_matrix((G.weight(200.0 * xi, 0), (ru, np.zeros(ru.size, dtype=np.int64))), shape=(2 * N, 1))
    S = sp.csr_matrix((G.weight(rs, cs), (rs, cs)), shape=(2 * N, m - 1))
    return U, S


def pattern_of(elements, m):
    """CSR pattern (indptr, indices; int32, sorted, diagonal included) of the level Hessian: union of the element cliques."""
    rows, cols = [], []
    for el in elements:
        a = np.asarray(el)
        rows.append(np.repeat(a, a.size)); cols.append(np.tile(a, a.size))
    P = sp.csr_matrix((np.ones(sum(r.size for r in rows)), (np.concatenate(rows), np.concatenate(cols))), shape=(m, m))
    P.sum_duplicates(); P.sort_indices()
    assert np.all(P.diagonal() > 0), "a column without an element"
    return P.indptr.astype(np.int32), P.indices.astype(np.int32)


def centroids(N, elements, m):
    """The ordering hint of mgbhip_problem::ensure_analysis: sum_i |R_ij| x_i / sum_i |R_ij| over the rows of R in order."""
    U, S = level_matrices(N, elements, m)
    R = sp.block_diag([U, S], format="csr")
    R.sort_indices()
    nodes = np.linspace(-1.0, 1.0, N + 1)
    x = np.stack([nodes[:-1], nodes[1:]], axis=1).reshape(-1)
    rows = np.repeat(np.arange(R.shape[0]), np.diff(R.indptr))
    a = np.abs(R.data)
    cen, wsum = np.zeros(m), np.zeros(m)
    np.add.at(wsum, R.indices, a)                      # unbuffered, in entry order: the same sums as the C++ loop
    np.add.at(cen, R.indices, a * x[rows % (2 * N)])
    return np.where(wsum > 0, cen / np.where(wsum > 0, wsum, 1.0), 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the launch plan on the CPU (oracle/csrc/mf_host.cpp: mf_host_launches)
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _host_lib():
    path = os.path.join(ROOT, "oracle", "_build", "libmf_host.so")
    if not os.path.exists(path):
        raise RuntimeError(f"{path} missing: run python __graft_entry__.py")
    lib = C.CDLL(path)
    lib.mf_host_launches.restype = C.c_int64
    lib.mf_host_launches.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    return lib


def rows_as_dicts(raw):
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from mgb_amd.device import DeviceProblem          # imports without a GPU: one decoding of the rows
    return DeviceProblem.launch_rows(raw)


def host_launches(indptr, indices, coords, lds_cap=128, inv_ok=True, env=None, with_fronts=False, with_order=False):
    """Launch rows (dicts, as DeviceProblem.solver_launches) of a pattern from the CPU build; env: switches for this call."""
    lib = _host_lib()
    n = indptr.size - 1
    saved = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        cap = 4096
        out = np.zeros(cap * ROW, dtype=np.int32)
        fr = np.zeros(4 * (n + 2), dtype=np.int32)
        nf = C.c_int64(0)
        order = np.zeros(n + 1, dtype=np.int32)
        co = np.ascontiguousarray(coords, dtype=np.float64)
        cnt = lib.mf_host_launches(n, indptr.ctypes.data, indices.ctypes.data, co.ctypes.data, 1, 0, lds_cap, int(inv_ok),
                                   out.ctypes.data, cap, fr.ctypes.data, n + 2, C.byref(nf), order.ctypes.data)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert 0 <= cnt <= cap, cnt
    rows = rows_as_dicts(out[:cnt * ROW])
    if with_order:
        return rows, fr[:4 * nf.value].reshape(-1, 4), order
    return (rows, fr[:4 * nf.value].reshape(-1, 4)) if with_fronts else rows


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

def _arrows(ks, s, copies=1):
    def build():
        b = Builder()
        for _ in range(copies):
            b.arrow(ks, s)
        return b
    return build


def _rows(*tuples):
    return rows_as_dicts(np.asarray(tuples, dtype=np.int64))


def _parts(*parts):
    """parts: (ks, s) block arrows, ("stars", k, s1, s2) and ("leaves", ks, s, count, k, t, groups)."""
    def build():
        b = Builder()
        for p in parts:
            if p[0] == "stars":                   # two stars of p[1] uncoupled columns with nested neighbourhoods S1 and S1 + S2:
                s1, s2 = b.cols(p[2]), b.cols(p[3])     # peeled as two fronts of p[1] pivots with diagonal pivot blocks
                b.clique(s1, s2)
                for c in b.cols(p[1]):
                    b.clique([c], s1)
                for c in b.cols(p[1]):
                    b.clique([c], s1, s2)
            elif p[0] == "leaves":                # an arrow (p[1], p[2]) with p[3] cliques of p[4] columns hung on p[5] separator columns
                sep = b.arrow(p[1], p[2])
                for i in range(p[3]):             # ... taken in turn from p[6] disjoint groups of separator columns
                    g = i % p[6]
                    b.clique(b.cols(p[4]), sep[g * p[5]:(g + 1) * p[5]])
            else:
                b.arrow(p[0], p[1])
        return b
    return build


@dataclass
class Case:
    name: str
    build: object                       # () -> Builder
    rows: list                          # the launch rows the level must get as shipped (lds_cap = 128, inverse path available)
    gates: tuple                        # the sides of the gate table (GATES) this case is there for
    switched: dict = field(default_factory=dict)     # ((env name, value), ...) -> rows under those switches (worker process)
    grades: tuple = GRADES
    fronts: tuple = ()                  # the plan's fronts as shipped: (level, m, k, children, how many), sorted


N_ELEMENTS = 258
OLD_BIG = (("MGBHIP_OLD_BIG", "1"),)
INV_ALWAYS = (("MGBHIP_INV_MIN_N", "0"),)
NO_WAVE = (("MGBHIP_NO_WAVE_SMALL", "1"),)
NO_MERGE = (("MGBHIP_NO_MERGE_GROUPS", "1"),)
NO_PACKED = (("MGBHIP_NO_PACKED_LEAVES", "1"),)

# Row columns: level first count cls max_m max_k max_child | tiny wave inv iface packed | assembly block0 backward | 0
# (assembly 1 gather 2 columns; block0 1 gather workgroup 2 mf_big_diag0 3 in step 0; backward 1 k8 2 k16 3 general).
# A block arrow of q cliques (k_i) under a separator s comes out as q - 1 leaf fronts (k_i, k_i + s + 1), the root
# (k_q + s, k_q + s + 1) -- the last clique is amalgamated into the separator's front (exact fit) -- and the 1 x 1 border front.
# Cliques whose unknowns have at most 48 neighbours are peeled first, one unknown per clique and round (case `tiny`).
CASES = [
    Case("tiny", _arrows([8] * 4, 4),
         _rows((0, 0, 4, 16, 13, 4, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0),
               (1, 4, 1, 32, 21, 20, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('tiny leaf m<=16, packed', 'an m<=16 front above level 0 (the border front: wave)', 'class 32, 4 children'),
         {NO_PACKED: _rows((0, 0, 4, 16, 13, 4, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
               (1, 4, 1, 32, 21, 20, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
          NO_WAVE: _rows((0, 0, 4, 16, 13, 4, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0),
               (1, 4, 1, 32, 21, 20, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 13, 4, 0, 4), (1, 21, 20, 4, 1), (2, 1, 1, 1, 1),)),
    Case("wave48", _arrows([30] * 3, 17),
         _rows((0, 0, 2, 48, 48, 30, 0, 0, 1, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 48, 48, 47, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 48 at m=48', 'wave<48> childless'),
         {NO_WAVE: _rows((0, 0, 2, 48, 48, 30, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 48, 48, 47, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 48, 30, 0, 2), (1, 48, 47, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds49", _arrows([31] * 3, 17),
         _rows((0, 0, 2, 64, 49, 31, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 64, 49, 48, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 64 at m=49',),
         fronts=((0, 49, 31, 0, 2), (1, 49, 48, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds64", _arrows([46] * 3, 17),
         _rows((0, 0, 2, 64, 64, 46, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 64, 64, 63, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 64 at m=64',),
         fronts=((0, 64, 46, 0, 2), (1, 64, 63, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds65", _arrows([47] * 3, 17),
         _rows((0, 0, 2, 88, 65, 47, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 88, 65, 64, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 88 at m=65 (packed LDS triangle)',),
         fronts=((0, 65, 47, 0, 2), (1, 65, 64, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds88", _arrows([60] * 3, 27),
         _rows((0, 0, 2, 88, 88, 60, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 88, 88, 87, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 88 at m=88',),
         fronts=((0, 88, 60, 0, 2), (1, 88, 87, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds89", _arrows([61] * 3, 27),
         _rows((0, 0, 2, 128, 89, 61, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 128, 89, 88, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 128 at m=89',),
         fronts=((0, 89, 61, 0, 2), (1, 89, 88, 2, 1), (2, 1, 1, 1, 1),)),
    Case("lds128", _arrows([100] * 2, 27),
         _rows((0, 0, 1, 128, 128, 100, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 1, 1, 128, 128, 127, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 128 at m=128',),
         fronts=((0, 128, 100, 0, 1), (1, 128, 127, 1, 1), (2, 1, 1, 1, 1),)),
    Case("big129", _arrows([100] * 2, 28),
         _rows((0, 0, 1, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 1, 1, 0, 129, 128, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('large-front path at m=129', 'substitution kernels (n < 1024)', 'childless large front', 'gather with 1 child'),
         {INV_ALWAYS: _rows((0, 0, 1, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 1, 1, 0, 129, 128, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
          OLD_BIG: _rows((0, 0, 1, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 1, 1, 0, 129, 128, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 1), (1, 129, 128, 1, 1), (2, 1, 1, 1, 1),)),
    Case("merged_mixed", _arrows([30, 31, 46, 47, 40], 17),
         _rows((0, 0, 4, 88, 65, 47, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 4, 1, 64, 58, 57, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 2: a merged launch with mixed m and k',),
         {NO_MERGE: _rows((0, 0, 1, 48, 48, 30, 0, 0, 1, 0, 0, 0, 0, 0, 3, 0),
               (0, 1, 2, 64, 64, 46, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 3, 1, 88, 65, 47, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 4, 1, 64, 58, 57, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 48, 30, 0, 1), (0, 49, 31, 0, 1), (0, 64, 46, 0, 1), (0, 65, 47, 0, 1), (1, 58, 57, 4, 1), (2, 1, 1, 1, 1),)),
    Case("merge255", _arrows([8] * 255 + [30, 30], 41),
         _rows((0, 0, 256, 88, 72, 30, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 256, 62, 64, 62, 20, 5, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 318, 1, 88, 72, 71, 63, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 319, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 2: count 255 joins the next class (4 count >= next.count)',),
         fronts=((0, 50, 4, 0, 255), (0, 72, 30, 0, 1), (1, 58, 16, 4, 55), (1, 62, 20, 5, 7), (2, 72, 71, 63, 1), (3, 1, 1, 1, 1),)),
    Case("merge256", _arrows([8] * 256 + [30, 30], 41),
         _rows((0, 0, 256, 64, 50, 4, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 256, 1, 88, 72, 30, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 257, 62, 64, 62, 20, 5, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 319, 1, 88, 72, 71, 63, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 320, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 2: count 256 stays',),
         fronts=((0, 50, 4, 0, 256), (0, 72, 30, 0, 1), (1, 58, 16, 4, 54), (1, 62, 20, 5, 8), (2, 72, 71, 63, 1), (3, 1, 1, 1, 1),)),
    Case("rule1_accept", _parts(([31, 32, 66, 66, 66], 62), ([33, 64, 65, 65, 65], 63), ([1, 10, 64, 64, 64], 64), ([100, 100, 100], 28), ([40, 40, 40, 40, 66], 62)),
         _rows((0, 0, 16, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 16, 5, 0, 200, 128, 4, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 21, 2, 0, 166, 165, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (3, 23, 1, 16, 1, 1, 5, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 1 accepted at lds_count = big count: LDS-sized fronts on the large-front kernels, mixed k and m',),
         {OLD_BIG: _rows((0, 0, 8, 128, 103, 40, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 8, 8, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 16, 1, 128, 128, 127, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 17, 4, 0, 200, 128, 4, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 21, 2, 0, 166, 165, 1, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (3, 23, 1, 16, 1, 1, 5, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
          NO_MERGE: _rows((0, 0, 1, 88, 76, 11, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 1, 7, 128, 103, 40, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 8, 8, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 16, 1, 128, 128, 127, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 17, 4, 0, 200, 128, 4, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 21, 2, 0, 166, 165, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (3, 23, 1, 16, 1, 1, 5, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 76, 11, 0, 1), (0, 94, 31, 0, 1), (0, 95, 32, 0, 1), (0, 97, 33, 0, 1), (0, 103, 40, 0, 4), (0, 129, 4, 0, 1), (0, 129, 57, 0, 1), (0, 129, 65, 0, 3), (0, 129, 66, 0, 1), (0, 129, 100, 0, 2), (1, 128, 127, 4, 1), (1, 129, 128, 2, 1), (1, 129, 128, 4, 1), (1, 191, 62, 4, 1), (1, 200, 34, 2, 1), (2, 129, 128, 1, 1), (2, 166, 165, 1, 1), (3, 1, 1, 5, 1),)),
    Case("rule1_count", _parts(([31, 32, 66, 66, 66], 62), ([33, 64, 65, 65, 65], 63), ([1, 10, 64, 64, 64], 64), ([100, 100, 100], 28), ([40, 40, 40, 40, 40, 66], 62)),
         _rows((0, 0, 9, 128, 103, 40, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 9, 8, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 17, 5, 0, 193, 128, 5, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 22, 2, 0, 146, 145, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (3, 24, 1, 16, 1, 1, 5, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 1 refused: lds_count = big count + 1',),
         fronts=((0, 76, 11, 0, 1), (0, 94, 31, 0, 1), (0, 95, 32, 0, 1), (0, 97, 33, 0, 1), (0, 103, 40, 0, 5), (0, 129, 9, 0, 1), (0, 129, 64, 0, 1), (0, 129, 65, 0, 3), (0, 129, 66, 0, 1), (0, 129, 100, 0, 2), (1, 128, 127, 4, 1), (1, 129, 128, 2, 1), (1, 129, 128, 5, 1), (1, 186, 62, 4, 1), (1, 193, 47, 2, 1), (2, 124, 123, 1, 1), (2, 146, 145, 1, 1), (3, 1, 1, 5, 1),)),
    Case("rule1_m32", _parts(([31, 32, 66, 66, 66], 62), ([33, 64, 65, 65, 65], 63), ([1, 10, 64, 64, 64], 64), ([3, 100, 100, 100], 28)),
         _rows((0, 0, 7, 128, 128, 64, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 7, 8, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 15, 4, 0, 129, 128, 4, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 19, 1, 16, 1, 1, 4, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('merge rule 1 refused: a group with m <= 32',),
         fronts=((0, 32, 3, 0, 1), (0, 66, 1, 0, 1), (0, 75, 10, 0, 1), (0, 94, 31, 0, 1), (0, 95, 32, 0, 1), (0, 97, 33, 0, 1), (0, 128, 64, 0, 1), (0, 129, 64, 0, 2), (0, 129, 65, 0, 2), (0, 129, 66, 0, 2), (0, 129, 100, 0, 2), (1, 129, 128, 3, 1), (1, 129, 128, 4, 3), (2, 1, 1, 4, 1),)),
    Case("n1023", _arrows([100] * 9 + [95], 28),
         _rows((0, 0, 9, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 9, 1, 128, 124, 123, 9, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('inv gate: n=1023 substitution', '9 children in an LDS front'),
         fronts=((0, 129, 100, 0, 9), (1, 124, 123, 9, 1), (2, 1, 1, 1, 1),)),
    Case("n1024", _arrows([100] * 9 + [96], 28),
         _rows((0, 0, 9, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 9, 1, 128, 125, 124, 9, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('inv gate: n=1024 inverse-based', 'block 0 in step 0'),
         {OLD_BIG: _rows((0, 0, 9, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 9, 1, 128, 125, 124, 9, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 9), (1, 125, 124, 9, 1), (2, 1, 1, 1, 1),)),
    Case("c23", _arrows([100] * 24, 28),
         _rows((0, 0, 23, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 23, 1, 0, 129, 128, 23, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 24, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('23 fronts: block 0 in step 0', 'column-tiled assembly, 23 children'),
         fronts=((0, 129, 100, 0, 23), (1, 129, 128, 23, 1), (2, 1, 1, 1, 1),)),
    Case("c24", _arrows([100] * 25, 28),
         _rows((0, 0, 24, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0),
               (1, 24, 1, 0, 129, 128, 24, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 25, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('24 fronts: mf_big_diag0',),
         {OLD_BIG: _rows((0, 0, 24, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 24, 1, 0, 129, 128, 24, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (2, 25, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 24), (1, 129, 128, 24, 1), (2, 1, 1, 1, 1),)),
    Case("d24", _arrows([60] * 25, 68),
         _rows((0, 0, 24, 0, 129, 60, 0, 0, 0, 1, 0, 0, 2, 2, 0, 0),
               (1, 24, 1, 0, 129, 128, 24, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 25, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('24 fronts of k = 60 within 2048 unknowns (zero-pivot placement under mf_big_diag0)',),
         fronts=((0, 129, 60, 0, 24), (1, 129, 128, 24, 1), (2, 1, 1, 1, 1),)),
    Case("gather7", _arrows([100] * 8, 28, 2),
         _rows((0, 0, 14, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 14, 2, 0, 129, 128, 7, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 16, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('gather with 7 children', 'block 0 by the gather workgroup'),
         {OLD_BIG: _rows((0, 0, 14, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 14, 2, 0, 129, 128, 7, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 16, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 14), (1, 129, 128, 7, 2), (2, 1, 1, 2, 1),)),
    Case("ch8", _arrows([100] * 9, 28, 2),
         _rows((0, 0, 16, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 16, 2, 0, 129, 128, 8, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 18, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('8 children: mf_big_gather',),
         {OLD_BIG: _rows((0, 0, 16, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 16, 2, 0, 129, 128, 8, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 18, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 16), (1, 129, 128, 8, 2), (2, 1, 1, 2, 1),)),
    Case("ch9", _arrows([100] * 10, 28),
         _rows((0, 0, 9, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 9, 1, 0, 129, 128, 9, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('9 children: column-tiled',),
         {OLD_BIG: _rows((0, 0, 9, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 9, 1, 0, 129, 128, 9, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (2, 10, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 129, 100, 0, 9), (1, 129, 128, 9, 1), (2, 1, 1, 1, 1),)),
    Case("edge10240", _arrows([100] * 8, 1279),
         _rows((0, 0, 8, 0, 1380, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 8, 6, 0, 1330, 50, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 14, 1, 0, 1280, 1279, 8, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (3, 15, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('max_child max_m = 8 x 1280 = 10 240: gather', 'k = 1279, m - k = 1: 40 pivot blocks'),
         grades=(0,),
         fronts=((0, 1380, 50, 0, 2), (0, 1380, 75, 0, 3), (0, 1380, 87, 0, 1), (0, 1380, 100, 0, 2), (1, 1293, 13, 1, 1), (1, 1305, 25, 1, 3), (1, 1330, 50, 1, 2), (2, 1280, 1279, 8, 1), (3, 1, 1, 1, 1),)),
    Case("edge10241", _arrows([100] * 7, 1462),
         _rows((0, 0, 7, 0, 1563, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 7, 4, 0, 1513, 50, 1, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 11, 1, 0, 1463, 1462, 7, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (3, 12, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('max_child max_m = 7 x 1463 = 10 241: column-tiled',),
         grades=(0,),
         fronts=((0, 1563, 50, 0, 2), (0, 1563, 75, 0, 2), (0, 1563, 100, 0, 3), (1, 1488, 25, 1, 2), (1, 1513, 50, 1, 2), (2, 1463, 1462, 7, 1), (3, 1, 1, 1, 1),)),
    Case("mixed_inv", _arrows([33, 64, 65, 31, 1, 100, 90, 100], 28, 2),
         _rows((0, 0, 12, 128, 119, 90, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 12, 2, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 14, 2, 0, 129, 128, 7, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 16, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('k = 1 ... 90 in one LDS launch beside large fronts',),
         {OLD_BIG: _rows((0, 0, 12, 128, 119, 90, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 12, 2, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 14, 2, 0, 129, 128, 7, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 16, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 30, 1, 0, 2), (0, 60, 31, 0, 2), (0, 62, 33, 0, 2), (0, 93, 64, 0, 2), (0, 94, 65, 0, 2), (0, 119, 90, 0, 2), (0, 129, 100, 0, 2), (1, 129, 128, 7, 2), (2, 1, 1, 2, 1),)),
    Case("wave_c8", _arrows([10] * 3, 7),
         _rows((0, 0, 2, 32, 18, 4, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 2, 1, 32, 20, 12, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 3, 1, 32, 18, 17, 1, 0, 1, 0, 0, 0, 0, 0, 3, 0),
               (3, 4, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('wave<32> with a child of m - k = 8',),
         {NO_WAVE: _rows((0, 0, 2, 32, 18, 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0),
               (1, 2, 1, 32, 20, 12, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 3, 1, 32, 18, 17, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 4, 1, 16, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 18, 4, 0, 2), (1, 20, 12, 2, 1), (2, 18, 17, 1, 1), (3, 1, 1, 1, 1),)),
    Case("wave_c9", _arrows([10] * 3, 8),
         _rows((0, 0, 2, 32, 19, 4, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 2, 1, 32, 21, 12, 2, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 3, 1, 32, 19, 18, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 4, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('child m - k = 9: mf_factor_small',),
         fronts=((0, 19, 4, 0, 2), (1, 21, 12, 2, 1), (2, 19, 18, 1, 1), (3, 1, 1, 1, 1),)),
    Case("k8", _parts(('stars', 8, 20, 5)),
         _rows((0, 0, 1, 32, 29, 8, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 1, 1, 48, 34, 33, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('LDS sweep max_k = 8: k8',),
         fronts=((0, 29, 8, 0, 1), (1, 34, 33, 1, 1), (2, 1, 1, 1, 1),)),
    Case("k9", _parts(('stars', 9, 20, 5)),
         _rows((0, 0, 1, 32, 30, 9, 0, 0, 1, 0, 0, 0, 0, 0, 2, 0),
               (1, 1, 1, 48, 35, 34, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 2, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('LDS sweep max_k = 9: k16',),
         fronts=((0, 30, 9, 0, 1), (1, 35, 34, 1, 1), (2, 1, 1, 1, 1),)),
    Case("k16", _arrows([16] * 3, 41),
         _rows((0, 0, 2, 64, 58, 16, 0, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (1, 2, 1, 64, 58, 57, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('LDS sweep max_k = 16: k16',),
         fronts=((0, 58, 16, 0, 2), (1, 58, 57, 2, 1), (2, 1, 1, 1, 1),)),
    Case("k17", _arrows([17] * 3, 41),
         _rows((0, 0, 2, 64, 59, 17, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 2, 1, 64, 59, 58, 2, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('LDS sweep max_k = 17: general',),
         fronts=((0, 59, 17, 0, 2), (1, 59, 58, 2, 1), (2, 1, 1, 1, 1),)),
    Case("ch16", _arrows([25] * 17, 30),
         _rows((0, 0, 16, 64, 56, 25, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 16, 1, 64, 56, 55, 16, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 17, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('16 children of an LDS front',),
         fronts=((0, 56, 25, 0, 16), (1, 56, 55, 16, 1), (2, 1, 1, 1, 1),)),
    Case("ch17", _arrows([25] * 18, 30),
         _rows((0, 0, 17, 64, 56, 25, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (1, 17, 1, 64, 56, 55, 17, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 18, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('17 children of an LDS front',),
         fronts=((0, 56, 25, 0, 17), (1, 56, 55, 17, 1), (2, 1, 1, 1, 1),)),
    Case("m16", _arrows([4] * 4, 11),
         _rows((0, 0, 4, 16, 16, 3, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0),
               (1, 4, 1, 16, 16, 15, 4, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 16 at m = 16: tiny leaves and a class-16 front above level 0',),
         {NO_WAVE: _rows((0, 0, 4, 16, 16, 3, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0),
               (1, 4, 1, 16, 16, 15, 4, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 16, 3, 0, 4), (1, 16, 15, 4, 1), (2, 1, 1, 1, 1),)),
    Case("m17", _arrows([4] * 4, 12),
         _rows((0, 0, 4, 32, 17, 3, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 4, 1, 32, 17, 16, 4, 0, 0, 0, 0, 0, 0, 0, 2, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 32 at m = 17',),
         fronts=((0, 17, 3, 0, 4), (1, 17, 16, 4, 1), (2, 1, 1, 1, 1),)),
    Case("m32", _arrows([4] * 4, 27),
         _rows((0, 0, 4, 32, 32, 3, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 4, 1, 32, 32, 31, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 32 at m = 32',),
         fronts=((0, 32, 3, 0, 4), (1, 32, 31, 4, 1), (2, 1, 1, 1, 1),)),
    Case("m33", _arrows([4] * 4, 28),
         _rows((0, 0, 4, 48, 33, 3, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0),
               (1, 4, 1, 48, 33, 32, 4, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 5, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('class 48 at m = 33',),
         fronts=((0, 33, 3, 0, 4), (1, 33, 32, 4, 1), (2, 1, 1, 1, 1),)),
    Case("k1_subst", _arrows([1, 1, 1], 200),
         _rows((0, 0, 2, 0, 203, 2, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 2, 1, 0, 201, 200, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('k = 1 on the large-front path, substitution kernels (n < 1024)',),
         {INV_ALWAYS: _rows((0, 0, 2, 0, 203, 2, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 2, 1, 0, 201, 200, 2, 0, 0, 1, 0, 0, 1, 1, 0, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 202, 1, 0, 1), (0, 203, 2, 0, 1), (1, 201, 200, 2, 1), (2, 1, 1, 1, 1),)),
    Case("k1_inv", _parts(([1, 100, 100], 130), ([100] * 9 + [96], 28)),
         _rows((0, 0, 12, 0, 231, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 12, 2, 0, 131, 130, 9, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 14, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('k = 1 (m = 132) in an inverse-based launch',),
         {OLD_BIG: _rows((0, 0, 1, 128, 125, 96, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 1, 11, 0, 231, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 12, 2, 0, 131, 130, 9, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (2, 14, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 125, 96, 0, 1), (0, 129, 100, 0, 8), (0, 132, 1, 0, 1), (0, 231, 100, 0, 2), (1, 129, 128, 9, 1), (1, 131, 130, 3, 1), (2, 1, 1, 2, 1),)),
    Case("k1_rule1", _parts(([1, 64, 64, 64], 64), ([100] * 9 + [96], 28)),
         _rows((0, 0, 12, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 12, 2, 0, 162, 128, 9, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 14, 1, 128, 98, 97, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 15, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('k = 1 (m = 66) folded by merge rule 1; k = 64 and 31 with m = 129',),
         {OLD_BIG: _rows((0, 0, 2, 128, 125, 96, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (0, 2, 10, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 12, 2, 0, 162, 128, 9, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (2, 14, 1, 128, 98, 97, 1, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (3, 15, 1, 16, 1, 1, 2, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 66, 1, 0, 1), (0, 125, 96, 0, 1), (0, 129, 31, 0, 1), (0, 129, 64, 0, 1), (0, 129, 100, 0, 8), (1, 129, 128, 9, 1), (1, 162, 64, 3, 1), (2, 98, 97, 1, 1), (3, 1, 1, 2, 1),)),
    Case("leaf_big_subst", _parts(('leaves', [100, 100], 28, 8, 1, 5, 1)),
         _rows((0, 0, 1, 16, 14, 8, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
               (0, 1, 1, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 2, 1, 0, 129, 128, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0),
               (2, 3, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('tiny leaves under a large-front parent: square, read by mf_big_gather',),
         fronts=((0, 14, 8, 0, 1), (0, 129, 100, 0, 1), (1, 129, 128, 2, 1), (2, 1, 1, 1, 1),)),
    Case("leaf_big_inv", _parts(('leaves', [100] * 10, 28, 30, 1, 5, 3)),
         _rows((0, 0, 3, 16, 16, 10, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
               (0, 3, 9, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 12, 1, 0, 129, 128, 12, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (2, 13, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('tiny leaves (m = 16) under a large-front parent: square, read by the column-tiled assembly',),
         {OLD_BIG: _rows((0, 0, 3, 16, 16, 10, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
               (0, 3, 9, 0, 129, 100, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (1, 12, 1, 0, 129, 128, 12, 0, 0, 0, 0, 0, 2, 0, 0, 0),
               (2, 13, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 16, 10, 0, 3), (0, 129, 100, 0, 9), (1, 129, 128, 12, 1), (2, 1, 1, 1, 1),)),
    Case("leaf_lds", _parts(('leaves', [100] * 9 + [99], 28, 30, 1, 5, 3)),
         _rows((0, 0, 3, 16, 16, 10, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0),
               (0, 3, 9, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 12, 1, 128, 128, 127, 12, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 13, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0)),
         ('the same leaves under a class-128 parent: packed',),
         {NO_PACKED: _rows((0, 0, 3, 16, 16, 10, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0),
               (0, 3, 9, 0, 129, 100, 0, 0, 0, 1, 0, 0, 2, 3, 0, 0),
               (1, 12, 1, 128, 128, 127, 12, 0, 0, 0, 0, 0, 0, 0, 3, 0),
               (2, 13, 1, 16, 1, 1, 1, 0, 1, 0, 0, 0, 0, 0, 1, 0))},
         fronts=((0, 16, 10, 0, 3), (0, 129, 100, 0, 9), (1, 128, 127, 12, 1), (2, 1, 1, 1, 1),)),
]
CASE = {c.name: c for c in CASES}


# ---------------------------------------------------------------------------------------------------------------------
# the hierarchy, the matrices, the exact residual
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def built(name):
    b = CASE[name].build()
    assert len(b.elements) <= N_ELEMENTS and b.m <= 3000
    return b


@functools.lru_cache(maxsize=None)
def pattern(name):
    b = built(name)
    return pattern_of(b.elements, b.m)


def host_rows(name, env=None, **kw):
    """Launch rows of a case from the CPU build (with_fronts=True: also its fronts)."""
    b = built(name)
    return host_launches(*pattern(name), centroids(N_ELEMENTS, b.elements, b.m), env=dict(env or ()), **kw)


@functools.lru_cache(maxsize=None)
def problem():
    """One fem1d hierarchy of N_ELEMENTS elements: level l is CASES[l], the last level the true finest one."""
    return G.fem1d_problem(N_ELEMENTS, [level_matrices(N_ELEMENTS, built(c.name).elements, built(c.name).m) for c in CASES])


LEVEL = {c.name: l for l, c in enumerate(CASES)}


@functools.lru_cache(maxsize=None)
def system(name, grade):
    """(A, g, x_true).  The core has off-diagonals +-weight in [0.3, 0.95] (seeded signs, symmetric) and diagonal = absolute row
    sum + 1; A = D core D with D = 10^uniform(-grade/2, grade/2) as solver_cases.graded_spd scales it.  x_true = D^-1 t with
    |t| in [0.5, 1.5] (grade 0: x_true = t): every term of a row of A x then has the size of the core's term times the row's
    own scale, which is what keeps a single lost term visible in eta at grade 12 (tests/test_solver_gate_cases.py)."""
    indptr, indices = pattern(name)
    m = indptr.size - 1
    rng = np.random.default_rng(1000 * LEVEL[name] + grade)
    rows = np.repeat(np.arange(m), np.diff(indptr))
    lo, hi = np.minimum(rows, indices), np.maximum(rows, indices)
    sign = np.where(rng.random((m, 1)) < 0.5, -1.0, 1.0) * np.where(rng.random((1, m)) < 0.5, -1.0, 1.0)     # rank-one: symmetric up to ...
    sgn = sign[lo, hi] * np.where((lo * 7919 + hi * 104729) % 3 == 0, -1.0, 1.0)                              # ... a fixed pair pattern
    v = np.where(rows == indices, 0.0, G.weight(3 * lo, hi) * sgn)
    core = sp.csr_matrix((v, indices, indptr), shape=(m, m))
    dia = np.asarray(abs(core).sum(axis=1)).ravel() + 1.0
    v = np.where(rows == indices, dia[rows], v)
    d = 10.0 ** rng.uniform(-grade / 2, grade / 2, m) if grade else np.ones(m)
    A = sp.csr_matrix((d[lo] * v * d[hi], indices.copy(), indptr.copy()), shape=(m, m))       # one rounding order for (i, j) and (j, i)
    assert abs(A - A.T).max() == 0.0
    t = rng.uniform(0.5, 1.5, m) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
    x_true = t / d
    return A, A @ x_true, x_true


def two_products(a, b):
    """(p, e) with a * b = p + e exactly (Veltkamp split and Dekker's product; no overflow or underflow at these magnitudes)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_residual(A, x, g):
    """A x - g with every row summed exactly and rounded once: each product is split into two doubles without error and
    math.fsum returns the correctly rounded sum of its arguments -- the value float(gate_cases.exact_sum(...)) gives (compared in
    tests/test_solver_gate_cases.py), at a cost that keeps the 4-million-entry levels of the 40 KiB pair within seconds."""
    import math
    p, e = two_products(A.data, x[A.indices])
    r = np.zeros(g.size)
    for i in range(g.size):
        q = slice(A.indptr[i], A.indptr[i + 1])
        r[i] = math.fsum(np.concatenate([p[q], e[q], [-g[i]]]).tolist())
    return r


def exact_residual_rational(A, x, g):
    """The same through gate_cases.exact_sum (Fractions): the slow twin that exact_residual is checked against."""
    r = np.zeros(g.size)
    for i in range(g.size):
        q = slice(A.indptr[i], A.indptr[i + 1])
        r[i] = float(G.exact_sum(np.concatenate([A.data[q], [-1.0]]), np.concatenate([x[A.indices[q]], [g[i]]])))
    return r


def denominators(A, x, g):
    return abs(A) @ np.abs(x) + np.abs(g)


def eta(A, x, g):
    """Oettli-Prager componentwise backward error with the exact residual."""
    return float(np.max(np.abs(exact_residual(A, x, g)) / denominators(A, x, g)))


@functools.lru_cache(maxsize=None)
def reference(name, grade):
    """x_ref: a SciPy solve and one refinement step on the exact residual."""
    import scipy.sparse.linalg as spla
    A, g, _ = system(name, grade)
    lu = spla.splu(sp.csc_matrix(A))
    x = lu.solve(g)
    return x - lu.solve(exact_residual(A, x, g))


# ---------------------------------------------------------------------------------------------------------------------
# worker process (the switches are read once per process): python solver_gate_cases.py OUT.npz CASE [CASE ...]
#                                                                   python solver_gate_cases.py OUT.npz zero TAG [TAG ...]
# ---------------------------------------------------------------------------------------------------------------------

def run_cases(P, names, out):
    """Both solve paths of every (case, grade), twice (bitwise determinism), and the launch rows after the first solve."""
    import json
    for name in names:
        lev = LEVEL[name]
        for grade in CASE[name].grades:
            A, g, _ = system(name, grade)
            key = f"{name}_g{grade}"
            for rep in ("", "_again"):
                P.set_hessian(lev, A.data)
                out[key + "_x" + rep] = P.solve(lev, g)
                P.set_hessian(lev, A.data)
                xn, lam, status = P.solve_newton(lev, g, check=False)
                out[key + "_xn" + rep], out[key + "_lam" + rep] = xn, np.array([lam, float(status)])
        ip, ix = P.hessian_pattern(lev)
        out[name + "_pattern_ok"] = np.array(np.array_equal(ip, pattern(name)[0]) and np.array_equal(ix, pattern(name)[1]))
        out[name + "_rows"] = np.array(json.dumps(P.solver_launches(lev)))


# ---------------------------------------------------------------------------------------------------------------------
# zero pivots inside each kernel family
# ---------------------------------------------------------------------------------------------------------------------

# (tag, case, (level, m, k) of the front, pivot inside it, what the placement is)
ZERO_PIVOTS = [
    ("tiny_last", "tiny", (0, 13, 4), 3, "the last pivot of a tiny leaf"),
    ("wave", "wave48", (0, 48, 30), 17, "a wave front (mf_factor_wave<48>)"),
    ("lds64_col8", "lds64", (0, 64, 46), 8, "column 8, the second 8-column panel, of a class-64 LDS front"),
    ("lds128_col8", "lds128", (0, 128, 100), 8, "column 8 of a class-128 LDS front"),
    ("block0_step0", "n1024", (0, 129, 100), 5, "block 0 factored inside step 0"),
    ("block0_diag0", "d24", (0, 129, 60), 5, "block 0 factored by mf_big_diag0"),
    ("block0_gather", "ch8", (1, 129, 128), 5, "block 0 factored by the gather workgroup"),
    ("pivot32", "n1024", (0, 129, 100), 32, "pivot 32: the first of the second 32-column block"),
    ("ragged_last", "n1024", (0, 129, 100), 99, "the last pivot of a ragged last block (k = 100)"),
]
ZERO = {z[0]: z for z in ZERO_PIVOTS}


@functools.lru_cache(maxsize=None)
def zero_pivot_system(tag):
    """(A, g, x_ref, j): the grade-0 matrix of the case with a_jj = 0 and explicit zeros for every coupling of unknown j -- pivot
    `pivot` of the first front of the given shape -- to unknowns eliminated before it (earlier pivots of its front, its
    subtree); the later couplings stay.  Pivot j of the un-pivoted LDL' is then exactly zero; the matrix is regular and
    indefinite.  x_ref: dense LU with partial pivoting."""
    _, name, shape, pivot, _ = ZERO[tag]
    b = built(name)
    _, fronts, order = host_launches(*pattern(name), centroids(N_ELEMENTS, b.elements, b.m), with_order=True)
    f = next(i for i, fr in enumerate(fronts.tolist()) if (fr[0], fr[1], fr[2]) == shape)
    off = int(fronts[:f, 2].sum())
    j = int(order[off + pivot])
    pos = np.empty(b.m + 1, dtype=np.int64)
    pos[order] = np.arange(b.m + 1)
    A, _, x_true = system(name, 0)
    A = A.copy()
    rows = np.repeat(np.arange(b.m), np.diff(A.indptr))
    kill = ((rows == j) & (pos[A.indices] <= pos[j])) | ((A.indices == j) & (pos[rows] <= pos[j]))
    assert np.any((rows == j) & ~kill), "no later coupling is left"
    A.data[kill] = 0.0                                   # explicit zeros keep their slot in the pattern
    assert b.m <= 2048, "the LU fallback holds systems of at most 2048 unknowns"
    Ad = A.toarray()
    assert np.linalg.cond(Ad) < 1e8, (tag, "the matrix must be regular")
    g = A @ x_true
    return A, g, np.linalg.solve(Ad, g), j


def run_zero_pivots(P, tags, out):
    """Both solve paths on the zero-pivot matrices: x and status (a raised MGBHipError is recorded as its status)."""
    from mgb_amd import device as dev
    for tag in tags:
        lev = LEVEL[ZERO[tag][1]]
        A, g, _, _ = zero_pivot_system(tag)
        P.set_hessian(lev, A.data)
        try:
            out[tag + "_x"], out[tag + "_status"] = P.solve(lev, g), np.array(0.0)
        except dev.MGBHipError as e:
            out[tag + "_x"], out[tag + "_status"] = np.full(g.size, np.nan), np.array(float(e.status))
        P.set_hessian(lev, A.data)
        xn, lam, status = P.solve_newton(lev, g, check=False)
        out[tag + "_xn"], out[tag + "_statusn"], out[tag + "_lam"] = xn, np.array(float(status)), np.array(lam)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    from mgb_amd.device import DeviceProblem, HipContext
    prob = problem()
    ctx = HipContext(0)
    P = DeviceProblem(ctx, prob.M[0], prob.Q)
    res = {}
    if sys.argv[2] == "zero":
        run_zero_pivots(P, sys.argv[3:], res)
    else:
        run_cases(P, sys.argv[2:], res)
    P.close()
    ctx.close()
    np.savez(sys.argv[1], **res)
