"""Hand-built two-level problems that put every element-kernel variant (csrc/elem_kernels.hpp; DESIGN.md "Element-kernel
dispatch") on its dispatch and workgroup edges, with references whose componentwise bounds come from error analysis.

Layout.  N elements of p nodes, `BlockDiag` operators of shape (p, p, N) written out as plain dataclasses like
dense_cases.built; nothing of the setup layer is called.  "id" is the exact identity; "d1" .. "d6" are synthetic blocks that
differ for EVERY element: entry (r, c) of element e = a(r) b(c) |weight(.. + 7 e)| rounded to 10 fractional bits, a and b fixed
mixed sign patterns.  u0, the columns of the coarse R and s carry the sign b(c) of their local node, so no row of D z cancels.
c and w differ per node and row; the slack row of c is negative (the terms of f0 do not cancel).  The slack of z0 is an integer
>= 8 |q|^p at every node, level and evaluation point (pieces with A, b: the same margin on A y + b; linear rows stay >= 64):
this file is about the machinery around the cone and the cone formulas at interior points, not about the cone wall.  The wall
itself (slack down to 2^-40 of s^(2/p), bounds that follow the conditioning of the residual) is tests/wall_cases.py.

Two levels per case: level 0 is R = blockdiag(dense rounded blocks), not a selection level (prolong kernel, real restriction,
diag_mask = 0); level 1 is the finest one: the identity for the slack states and for u a selection with empty rows (local
node pattern `node % 5 == 2`, Dirichlet-style: zsel = -1), every column with exactly one row, so the assembled Hessian of
that level holds the element blocks themselves, entry for entry.

Everything is a multiple of 2^-10 (s of the trial point: 2^-11), so z0 + R s and D (z0 + R s) are exact in fp64 in any order.

References (u = 2^-53; the cone's per-node gradient and Hessian come from the oracle in fp64, the sums around them are formed
in the 80-bit np.longdouble or exactly in rationals, dense_cases._x):
  Dz                        exact, bit for bit
  F, slack per node         the oracle, 1e-12 relative (as test_gpu_dense)
  f0, trial y               math.fsum of the per-node terms, KERNEL_RTOL relative; sum |term| <= 4 |sum term| is checked
  f1, trial g   finest      sum_k D_k' Y_k per element,   bound ((p + nD + 2) u + KERNEL_RTOL) sum |terms|
                coarse      + the restriction bound of gate_cases, ((len_j + 2) u + KERNEL_RTOL) sum_i |R_ij ret_i|
  f2            finest      sum D_k[rr,i] Y[rr][k,k2] D_k2[rr,j], bound ((T + 3) u + KERNEL_RTOL) sum |terms|, T the entry's
                            number of triple products (any summation order, the fast kernels' two-stage sum included)
                coarse      R' H_blk R: + ((T + 2) u + KERNEL_RTOL) sum |R_ai H_ab R_bj|, T its number of terms
An entry is checked only if its smallest non-zero term is >= SENSITIVITY x its bound; at most MAX_SKIPPED of a case's entries
may miss that, none in the first and last element of a workgroup or in row / column p - 1 of an element."""
import functools
import math
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

from dense_cases import ONE, UREF, _f, _x, rnd, sign
from gate_cases import KERNEL_RTOL, SENSITIVITY, U53, weight

MODES = ("f0", "f1", "f2", "node_F", "node_slack", "f01")
FAST_TABLE = ((4, 7), (3, 2), (5, 8), (4, 6), (7, 7), (6, 2), (8, 8), (7, 6))       # csrc/elem_layout.hpp: ELEM_FAST_TABLE
KIND_EP, KIND_LINEAR = 1, 2
NARROW_W = 4
TRIAL_STEP = 0.5


# ---------------------------------------------------------------------------------------------------------------------
# the gate arithmetic of csrc/elem_layout.hpp and problem.cpp, restated
# ---------------------------------------------------------------------------------------------------------------------

def elem_group(p):
    g = 1
    while g < p:
        g <<= 1
    return max(g, 2)


def lds_bytes(threads, p, nu, nD, nstage, mode):
    y = threads * nD if mode in ("f1", "f01") else threads * (nD * (nD + 1) // 2) if mode == "f2" else 0
    return max(threads * nu + nstage * (threads // elem_group(p)) * p * p + y, 256) * 8


def stage_fits(p, nu, nD, nstage, wide):
    tiles = nstage * (256 // elem_group(p)) * p * p * 8
    return tiles <= 64 * 1024 and lds_bytes(128 if wide else 256, p, nu, nD, nstage, "f2") <= 150 * 1024


def restated_plan(case, mode):
    """What mgbhip_elem_plan must report for `mode`, from the case's shape alone."""
    p, nu, nD = case.p, case.nu, case.nD
    wide = nD > 10 or any(k == KIND_EP and len(idx) > NARROW_W for k, idx, _ in case.pieces)
    slot, stage, nstage = {}, [], 0
    for _, name in case.D_full:
        if name == "id":
            stage.append(-1)
            continue
        if name not in slot:
            if stage_fits(p, nu, nD, nstage + 1, wide):
                slot[name] = nstage
                nstage += 1
            else:
                slot[name] = -2
        stage.append(slot[name])
    ymask = 0
    for _, idx, _ in case.pieces:
        for i in idx:
            ymask |= 1 << i
    if case.phase1:
        for k in range(case.NC - 1, nD):
            ymask |= 1 << k
    unstaged = sum(s == -2 for s in stage)
    default = (nu == 2 and ymask == (((1 << nD) - 1) & ~1)
               and all(a == (1 if k == nD - 1 else 0) for k, (a, _) in enumerate(case.D_full))
               and all(s == (-1 if k in (0, nD - 1) else k - 1) for k, s in enumerate(stage)))
    threads = 128 if (wide and mode == "f2") else 256
    G = elem_group(p)
    EPB = threads // G
    lds = lds_bytes(threads, p, nu, nD, nstage, mode)
    out = dict(threads=threads, G=G, EPB=EPB, grid=-(-case.N // EPB), lds=lds, nstage=nstage, unstaged=unstaged, ymask=ymask)
    if wide:
        out.update(kind="wide", NY=0, P=0)
    elif mode in ("f2", "f01") and (nD, p) in FAST_TABLE and unstaged == 0 and lds <= 160 * 1024:
        out.update(kind="fast_default" if default else "fast_runtime", NY=nD, P=p)
    else:
        out.update(kind="generic", NY=nD, P=0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    p: int
    N: int
    D_spec: list                       # [(state, operator name)] of the user problem
    pieces: list                       # [(kind, idx, options)], options: "A" (non-identity A, b grids), "pgrid" (per-node p)
    claims: dict                       # the plan the case must report, literal; checked by check_claims
    phase1: bool = False               # the phase-I image: one more state, rows [.., (nu, id), (0, id) .. (nu-1, id)]
    masked: bool = False               # barrier weights with zeros, half of them at nodes outside the cone
    select: bool = False               # a select grid with some nodes off

    @property
    def nu0(self):
        return 1 + max(a for a, _ in self.D_spec)

    @property
    def nu(self):
        return self.nu0 + (1 if self.phase1 else 0)

    @property
    def D_full(self):
        if not self.phase1:
            return list(self.D_spec)
        return list(self.D_spec) + [(self.nu0, "id")] + [(a, "id") for a in range(self.nu0)]

    @property
    def nD(self):
        return len(self.D_full)

    @property
    def NC(self):
        return len(self.D_spec) + 1 if self.phase1 else 0

    @property
    def n(self):
        return self.p * self.N

    @property
    def slack_states(self):
        s = [self.nu0 - 1] if self.nu0 > 1 else []
        return s + ([self.nu0] if self.phase1 else [])


def _d(*names, nu=2):
    """[u id, u <names> .., s id]"""
    return [(0, "id")] + [(0, nm) for nm in names] + [(nu - 1, "id")]


def _claims(f2, other, G, EPB, grid, nstage, unstaged=0, **kw):
    return dict(f2=f2, other=other, G=G, EPB=EPB, grid=grid, nstage=nstage, unstaged=unstaged, **kw)


EP = KIND_EP
LIN = KIND_LINEAR
_D3 = _d("d1")
_D4 = _d("d1", "d2")
_D5 = _d("d1", "d2", "d3")
_D7 = _d("d1", "d2", "d3", "d4", "d5")
_D9 = [(0, "id"), (0, "d1"), (0, "d2"), (0, "d3"), (0, "d1"), (0, "d2"), (0, "d3"), (0, "id"), (1, "id")]
_D10 = [(0, "id"), (0, "d1"), (0, "d2"), (0, "d3"), (0, "d4"), (0, "d5"), (0, "d6"), (0, "d1"), (0, "id"), (1, "id")]
_W7 = [(0, "id"), (0, "d1"), (0, "d2"), (1, "id"), (1, "d1"), (1, "d2"), (2, "id")]
_W11 = [(0, "id"), (0, "d1"), (0, "d2"), (0, "d3"), (1, "id"), (1, "d1"), (1, "d2"), (1, "d3"), (0, "d4"), (1, "d4"), (2, "id")]
_W13 = [(a, nm) for a in range(3) for nm in ("id", "d1", "d2", "d3")] + [(3, "id")]
_P3 = [(EP, (1, 2), "")]
_P4 = [(EP, (1, 2, 3), "")]
_P5 = [(EP, (1, 2, 3, 4), "")]
_PW7 = (1, 2, 4, 5, 6)

CASES = [
    # fem1d shape: fast (3, 2) with the default signature; one full workgroup plus one element, exactly one, a single element
    Case("p2_default", 2, 129, _D3, _P3, _claims(("fast_default", 3, 2), ("generic", 3, 0), 2, 128, 2, 1)),
    Case("p2_default_n128", 2, 128, _D3, _P3, _claims(("fast_default", 3, 2), ("generic", 3, 0), 2, 128, 1, 1)),
    Case("p2_default_n1", 2, 1, _D3, _P3, _claims(("fast_default", 3, 2), ("generic", 3, 0), 2, 128, 1, 1)),
    # the same rows permuted: the runtime signature of the same (NY, P)
    Case("p2_dx_first", 2, 129, [(0, "d1"), (0, "id"), (1, "id")], [(EP, (0, 2), "")],
         _claims(("fast_runtime", 3, 2), ("generic", 3, 0), 2, 128, 2, 1)),
    # fem2d_P2 with bubble: G = 8, one idle lane per element
    Case("p7_default", 7, 33, _D4, _P4, _claims(("fast_default", 4, 7), ("generic", 4, 0), 8, 32, 2, 2)),
    Case("p7_default_n32", 7, 32, _D4, _P4, _claims(("fast_default", 4, 7), ("generic", 4, 0), 8, 32, 1, 2)),
    # default signature, cone through piece_accumulate: per-node A, b and p
    Case("p7_general_cone", 7, 33, _D4, [(EP, (1, 2, 3), "A pgrid")], _claims(("fast_default", 4, 7), ("generic", 4, 0), 8, 32, 2, 2)),
    Case("p7_ymask", 7, 33, _D4, [(EP, (2, 3), "")], _claims(("fast_runtime", 4, 7), ("generic", 4, 0), 8, 32, 2, 2)),
    Case("p8_q1", 8, 33, _D5, _P5, _claims(("fast_default", 5, 8), ("generic", 5, 0), 8, 32, 2, 3)),
    Case("p6", 6, 33, _D4, _P4, _claims(("fast_default", 4, 6), ("generic", 4, 0), 8, 32, 2, 2)),
    # phase-I images: cobarrier and box terms, runtime signature
    Case("p2_default_phase1", 2, 129, _D3, _P3, _claims(("fast_runtime", 6, 2), ("generic", 6, 0), 2, 128, 2, 1), phase1=True),
    Case("p7_default_phase1", 7, 33, _D4, _P4, _claims(("fast_runtime", 7, 7), ("generic", 7, 0), 8, 32, 2, 2), phase1=True),
    Case("p8_q1_phase1", 8, 33, _D5, _P5, _claims(("fast_runtime", 8, 8), ("generic", 8, 0), 8, 32, 2, 3), phase1=True),
    Case("p6_phase1", 6, 33, _D4, _P4, _claims(("fast_runtime", 7, 6), ("generic", 7, 0), 8, 32, 2, 2), phase1=True),
    # the default-signature instantiation of (7, 7), which no discretisation reaches; 5 operators: the staging limit at p = 7
    Case("p7_two_piece_default", 7, 33, _D7, [(EP, (1, 2, 6), ""), (LIN, (3, 4, 5), "")],
         _claims(("fast_default", 7, 7), ("generic", 7, 0), 8, 32, 2, 5, stage_limit=5)),
    # an (8, 8) shape refused by the fast table: the fifth operator does not fit LDS and is read from HBM beside four staged
    Case("p8_unstaged", 8, 33, [(0, "id")] + [(0, f"d{i}") for i in range(1, 6)] + [(0, "id"), (1, "id")],
         [(EP, (1, 2, 7), ""), (LIN, (3, 4, 5), "")], _claims(("generic", 8, 0), ("generic", 8, 0), 8, 32, 2, 4, 1, stage_limit=4)),
    # generic<NY> at both ends of its range; idle lanes (G = 4 at p = 3, G = 8 at p = 5)
    Case("ny1", 3, 65, [(0, "id")], [(LIN, (0,), "")], _claims(("generic", 1, 0), ("generic", 1, 0), 4, 64, 2, 0)),
    Case("ny2", 3, 65, [(0, "d1"), (1, "id")], [(EP, (0, 1), "")], _claims(("generic", 2, 0), ("generic", 2, 0), 4, 64, 2, 1)),
    Case("ny9", 3, 65, _D9, [(EP, (1, 2, 3, 8), ""), (EP, (4, 5, 8), ""), (LIN, (6, 7, 0), "")],
         _claims(("generic", 9, 0), ("generic", 9, 0), 4, 64, 2, 3), select=True),
    # NY = 10 at p = 5: the f2 working-set term of elem_stage_fits decides (5 of 6 operators staged)
    Case("ny10", 5, 33, _D10, [(EP, (1, 2, 3, 9), ""), (EP, (4, 5, 9), ""), (LIN, (6, 7, 8), "")],
         _claims(("generic", 10, 0), ("generic", 10, 0), 8, 32, 2, 5, 1, stage_limit=5), select=True),
    Case("p1", 1, 129, [(0, "d1"), (1, "id")], [(EP, (0, 1), "")], _claims(("generic", 2, 0), ("generic", 2, 0), 2, 128, 2, 1)),
    Case("p9_q2", 9, 17, _D4, _P4, _claims(("generic", 4, 0), ("generic", 4, 0), 16, 16, 2, 2)),
    # operator tiles of exactly 64 KiB are staged (<=); a second operator is not
    Case("p32_tile_edge", 32, 9, _D3, _P3, _claims(("generic", 3, 0), ("generic", 3, 0), 32, 8, 2, 1, stage_limit=1)),
    Case("p32_two_ops", 32, 9, _D4, _P4, _claims(("generic", 4, 0), ("generic", 4, 0), 32, 8, 2, 1, 1, stage_limit=1)),
    Case("p33_mixed", 33, 5, _D4, _P4, _claims(("generic", 4, 0), ("generic", 4, 0), 64, 4, 2, 1, 1, stage_limit=1)),
    # wide kernels: f2 at 128 threads (EPB 32, grid 3), every other mode at 256 (EPB 64, grid 2)
    Case("wide_nd7", 4, 65, _W7, [(EP, _PW7, "")], _claims(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3)),
    Case("wide_A", 4, 65, _W7, [(EP, _PW7, "A")], _claims(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3)),
    Case("wide_nd11_narrow_cone", 4, 65, _W11, [(EP, (1, 2, 3, 10), ""), (EP, (5, 6, 7, 10), ""), (LIN, (8, 9, 0, 4), "")],
         _claims(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 4, f2_EPB=32, f2_grid=3)),
    Case("wide_nd7_phase1", 4, 65, _W7, [(EP, _PW7, "")], _claims(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3),
         phase1=True),
    Case("wide_nd13", 8, 17, _W13, [(EP, (1, 2, 3, 5, 6, 7, 9, 10, 11, 12), "")],
         _claims(("wide", 0, 0), ("wide", 0, 0), 8, 32, 1, 3, f2_EPB=16, f2_grid=2)),
    # masked nodes, half of them outside the cone: every output finite, their contribution exactly 0
    Case("p6_masked", 6, 33, _D4, _P4, _claims(("fast_default", 4, 6), ("generic", 4, 0), 8, 32, 2, 2), masked=True),
]
CASE = {c.name: c for c in CASES}
LEVELS = [(c.name, l) for c in CASES for l in (0, 1)]
WORKER_CASES = ("p2_default", "p7_default", "wide_nd7")


def check_claims(case):
    """Every literal of `claims` against the restated gate arithmetic: a later edit of the staging rule or the fast table
    cannot let a case slip off its edge unnoticed."""
    cl = case.claims
    for mode in MODES:
        r = restated_plan(case, mode)
        want = cl["f2"] if mode in ("f2", "f01") else cl["other"]
        assert (r["kind"], r["NY"], r["P"]) == want, (case.name, mode, r, want)
        assert r["G"] == cl["G"] and r["nstage"] == cl["nstage"] and r["unstaged"] == cl["unstaged"], (case.name, mode, r)
        wide_f2 = r["kind"] == "wide" and mode == "f2"
        assert r["EPB"] == (cl["f2_EPB"] if wide_f2 else cl["EPB"]), (case.name, mode, r)
        assert r["grid"] == (cl["f2_grid"] if wide_f2 else cl["grid"]), (case.name, mode, r)
        assert r["lds"] <= 160 * 1024, (case.name, mode, r)
    if "stage_limit" in cl:          # the largest number of operators elem_stage_fits accepts for this shape
        wide = restated_plan(case, "f2")["kind"] == "wide"
        k = 0
        while stage_fits(case.p, case.nu, case.nD, k + 1, wide):
            k += 1
        assert k == cl["stage_limit"], (case.name, k)
    return True


for _c in CASES:
    check_claims(_c)


def expected_plan(name, mode):
    """The fields test_gpu_elem asserts against DeviceProblem.elem_plan(mode)."""
    return restated_plan(CASE[name], mode)


# ---------------------------------------------------------------------------------------------------------------------
# the problems
# ---------------------------------------------------------------------------------------------------------------------

_OP_SALT = {f"d{i}": (0.4 + 2.5 * i, 11 + 6 * i, i) for i in range(1, 7)}


def operator(name, p, N):
    """(N, p, p) blocks [e, r, c]; every element's block is different."""
    e, r, c = np.arange(N)[:, None, None], np.arange(p)[None, :, None], np.arange(p)[None, None, :]
    if name == "id":
        return np.broadcast_to(np.eye(p), (N, p, p)).copy()
    sa, f, j0 = _OP_SALT[name]
    return sign(r, sa) * sign(c, 1.3) * rnd(weight(f * r + 3 * c + 7 * e, j0 + e))


def empty_row(node):
    return node % 5 == 2


@dataclass
class Built:
    case: Case
    D: list                            # nD arrays (N, p, p)
    state: list
    R: list                            # per level: csr (nu n x m)
    sel: np.ndarray                    # finest level: column of every row of R, -1 for an empty row
    s: list                            # per level: the level's vector (the iterate x of the trial)
    dirs: list                         # per level: the trial's direction
    z0: np.ndarray
    w: np.ndarray
    c: np.ndarray
    bw: object
    box: tuple
    outside: np.ndarray                # masked case: the masked nodes whose point lies outside the cone
    M: object = field(repr=False, default=None)
    Q: object = field(repr=False, default=None)
    Qo: object = field(repr=False, default=None)       # the oracle's functor (FeasConvex for phase I)


def masked_nodes(case):
    p, n = case.p, case.n
    epb = 256 // elem_group(p)
    return sorted({0, p - 1, p, n - 1, epb * p - 1, epb * p, 2 * p + 1, 3 * p + 2})


@functools.lru_cache(maxsize=None)
def built(name):
    from mgb_amd.blockmatrices import BlockColumn, BlockDiag
    from mgb_amd.convex import Convex, Piece
    from mgb_amd.multigrid import AMG, Geometry
    from oracle import mgb_oracle as O
    case = CASE[name]
    p, N, n, nu, nD = case.p, case.N, case.n, case.nu, case.nD
    nodes = np.arange(n)
    loc = nodes % p
    names = sorted({nm for _, nm in case.D_full})
    ops = {nm: operator(nm, p, N) for nm in names}
    D = [ops[nm] for _, nm in case.D_full]
    state = [a for a, _ in case.D_full]
    slack = case.slack_states
    # level 0: blockdiag of dense rounded blocks (3 columns per u state, 2 per slack state); level 1: selection / identity
    blocks0, sg0, blocks1, sel = [], [], [], []
    col1 = 0
    for a in range(nu):
        cw = 2 if a in slack else 3
        i = np.arange(cw)[None, :]
        k = nodes[:, None]
        if a in slack:
            blocks0.append(sign(k, 0.7) * sign(i, 2.2) * rnd(weight(7 * k + 2, 5 * i + 3 + a)))
            sg0.append(sign(np.arange(cw), 2.2))
            rows = nodes
        else:
            blocks0.append(sign(loc[:, None], 1.3) * sign(i, 0.9 + 2.0 * a) * rnd(weight(11 * k + 5, 3 * i + 0.9 + 2.0 * a)))
            sg0.append(sign(np.arange(cw), 0.9 + 2.0 * a))
            rows = nodes[~empty_row(nodes)]
        sa = np.full(n, -1, dtype=np.int64)
        sa[rows] = col1 + np.arange(rows.size)
        sel.append(sa)
        blocks1.append(sp.csr_matrix((np.ones(rows.size), (rows, np.arange(rows.size))), shape=(n, rows.size)))
        col1 += rows.size
    sel = np.concatenate(sel)
    R = [sp.csr_matrix(sp.block_diag(blocks0)), sp.csr_matrix(sp.block_diag(blocks1))]
    sg = np.concatenate(sg0)
    s0 = sg * (1 + np.arange(sg.size) % 3) / ONE
    d0 = sg * (2 + np.arange(sg.size) % 2) / ONE * np.where(np.arange(sg.size) % 2, 1.0, -1.0)
    rows1 = np.flatnonzero(sel >= 0)
    st1 = rows1 // n
    sg1 = np.where(np.isin(st1, slack), sign(rows1 % n, 0.7), sign((rows1 % n) % p, 1.3))
    s1 = sg1 * (1 + np.arange(rows1.size) % 3) / ONE
    d1 = sg1 * (2 + np.arange(rows1.size) % 2) / ONE * np.where(np.arange(rows1.size) % 3 == 1, -1.0, 1.0)
    svec, dirs = [s0, s1], [d0, d1]
    # z0: u states with the sign of their local node; slack states integers (set below); the phase-I slack small integers
    z0 = np.zeros(nu * n)
    for a in range(nu):
        if a not in slack:
            z0[a * n:(a + 1) * n] = sign(loc, 1.3) * rnd(weight(3 * nodes + 40 * a, 1 + a) / 8)
    if case.phase1:
        z0[case.nu0 * n:(case.nu0 + 1) * n] = 2.0 + nodes % 3
    # the cone: pieces over the user rows
    pcs = []
    pnode = np.array([1.5, 2.0, 3.0])[nodes % 3]
    for kind, idx, opt in case.pieces:
        ni = len(idx)
        if kind == EP:
            A = np.tile(np.eye(ni).reshape(-1, order="F"), (n, 1))
            b = np.zeros((n, ni))
            if "A" in opt:      # q rows: I + mixed-sign couplings among the q columns; s row: a_ss in [0.5, 0.95] on the slack alone
                Am = np.zeros((n, ni, ni))
                for r in range(ni - 1):
                    for cc in range(ni - 1):
                        Am[:, r, cc] = (1.0 if r == cc else 0.0) + sign(nodes + 3 * r, 0.5 + cc) * rnd(weight(5 * nodes + r, cc + 2) / 4)
                Am[:, ni - 1, ni - 1] = np.maximum(rnd(weight(3 * nodes, 7)), 0.5)
                A = Am.transpose(0, 2, 1).reshape(n, ni * ni)              # column-major flattened: [r + ni c]
                b[:, :ni - 1] = sign(nodes[:, None], 2.1) * rnd(weight(nodes[:, None], np.arange(ni - 1)[None, :]) / 4)
                b[:, ni - 1] = 1.0 + nodes % 2
            pg = pnode if "pgrid" in opt else np.full(n, 1.5)
            pcs.append(Piece(KIND_EP, tuple(idx), A, b, pg, np.where(pg < 2, 1.0, 2.0)))
        else:
            r_, c_ = np.arange(ni)[None, :, None], np.arange(ni)[None, None, :]
            Am = sign(nodes[:, None, None] + r_, 0.8 + c_) * rnd(weight(2 * nodes[:, None, None] + 3 * r_, c_ + 1))
            pcs.append(Piece(KIND_LINEAR, tuple(idx), Am.transpose(0, 2, 1).reshape(n, ni * ni), np.zeros((n, ni))))
    select = None
    if case.select:
        select = np.ones((n, len(pcs)))
        for k in range(len(pcs)):
            select[nodes % (5 + k) == 3, k] = 0.0
    Q = Convex(pcs, select)
    b = Built(case, D, state, R, sel, svec, dirs, z0, None, None, None, (1.0, 1.0), np.zeros(0, dtype=np.int64))
    # margins: Dz of the u rows at every level and evaluation point with the slack rows still zero
    ys = [dz_at(b, l, pt) for l in (0, 1) for pt in ("base", "trial")]
    base = 1.0
    for pc in pcs:
        if pc.kind == KIND_EP:
            for y in ys:
                _, q, _ = O._ep_parts(pc, y)
                need = 8.0 * np.max(np.maximum(np.sqrt(np.sum(q * q, axis=1)), 1.0) ** pc.p) + 2.0
                base = max(base, need)
        else:
            lo = min(float(np.min(np.einsum("nrc,nc->nr", pc.A.reshape(n, pc.ni, pc.nc).transpose(0, 2, 1), y[:, list(pc.idx)])))
                     for y in ys)
            pc.b[:] = (math.ceil(-lo) + 64.0 + (nodes % 3))[:, None]      # 64: |g| / n stays below |w c|, no entry of Y crosses zero
    base = 2.0 ** math.ceil(math.log2(base))
    if case.nu0 > 1:
        z0[(case.nu0 - 1) * n:case.nu0 * n] = base + 4.0 * (nodes % 5)
    if case.masked:
        mk = masked_nodes(case)
        bw = np.round(weight(5 * nodes, 2) * 64) / 16384
        bw[mk] = 0.0
        b.bw = bw
        b.outside = np.array(mk[::2], dtype=np.int64)
        z0[(case.nu0 - 1) * n + b.outside] = -3.0
    if case.phase1:
        zmax = float(np.abs(z0).max()) + 1.0
        b.box = (2.0 ** math.ceil(math.log2(2 * zmax)), 2.0 ** math.ceil(math.log2(4 * zmax)))
        b.Qo = O.FeasConvex(Q, b.box[0], b.box[1], case.NC)
    else:
        b.Qo = Q
    b.w = np.round(weight(nodes, 2) * ONE) / (ONE * 256)
    c = np.stack([sign(nodes, 0.3 + k) * rnd(weight(2 * nodes + k, k + 4)) for k in range(nD)], axis=1)
    for k in range(nD):
        if state[k] in slack:
            c[:, k] = -np.abs(c[:, k])          # slack rows: the linear part has the sign of the barrier (f0 does not cancel)
    b.c = c
    blk = {nm: BlockDiag(np.ascontiguousarray(ops[nm].transpose(1, 2, 0))) for nm in names}
    x = np.cos(0.37 * nodes + 0.1).reshape(n, 1)
    geom = Geometry(discretization=None, t=nodes.reshape(N, p).T.copy(), x=x.reshape(N, p, 1).transpose(1, 0, 2).copy(), w=b.w,
                    operators=blk)
    b.M = AMG(geometry=geom, x=x.copy(), w=b.w, R_fine=R, D_fine=[BlockColumn(blk[nm], a, nu) for a, nm in case.D_full],
              state_names=[f"v{a}" for a in range(nu)], D_spec=list(case.D_full))
    b.Q = Q
    return b


def point(b, level, pt):
    """The level's vector at an evaluation point: "base" = s, "trial" = s - TRIAL_STEP dir (exact)."""
    return b.s[level] if pt == "base" else b.s[level] - TRIAL_STEP * b.dirs[level]


def dz_at(b, level, pt):
    """Dz (n x nD) at a point, in fp64: every product and sum is exact (multiples of 2^-31 below 2^12), so this is the exact
    value in any summation order; checked against the 80-bit / rational sum."""
    case = b.case
    n, N, p = case.n, case.N, case.p
    z = b.z0 + b.R[level] @ point(b, level, pt)
    zx = _x(b.z0) + _x(np.asarray(b.R[level].todense())) @ _x(point(b, level, pt)) if n <= 64 else None
    if zx is not None:
        assert np.array_equal(_f(zx), z)
    Dz = np.empty((n, len(b.D)))
    for k, Dk in enumerate(b.D):
        zk = z[b.state[k] * n:(b.state[k] + 1) * n].reshape(N, p)
        Dz[:, k] = np.einsum("erc,ec->er", Dk, zk).reshape(n)
        chk = _f(np.einsum("erc,ec->er", _x(Dk[:2]), _x(zk[:2])))
        assert np.array_equal(chk.reshape(-1), Dz[:2 * p, k][:chk.size])
    return Dz


def inputs(name, level):
    b = built(name)
    return b.s[level], b.c, b.z0


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Reference:
    """value, componentwise bound, sum of |terms| and smallest non-zero |term| per entry, in the shape of the device's output;
    never: entries that may not miss the sensitivity condition."""
    value: np.ndarray
    bound: np.ndarray
    abssum: np.ndarray
    minterm: np.ndarray
    never: np.ndarray

    @property
    def sensitive(self):
        return self.minterm >= SENSITIVITY * self.bound

    @property
    def skipped(self):
        live = self.abssum > 0
        return 1.0 - float(self.sensitive[live].mean()) if live.any() else 0.0

    def ratios(self, device_values):
        d = np.asarray(device_values, dtype=np.float64).reshape(self.value.shape)
        empty = self.abssum == 0
        assert np.all(d[empty] == 0.0), "an entry with no term must be exactly zero"
        use = self.sensitive & ~empty
        r = np.abs(d[use] - self.value[use]) / self.bound[use]
        return np.where(np.isfinite(d[use]), r, np.inf)


MUTATIONS = ("op_shift", "z_shift", "drop_last_node", "swap_Y", "drop_term", "double_term", "unmask")


def applies(case, mut):
    if mut == "op_shift":
        return case.N > 1 and any(nm != "id" for _, nm in case.D_full)
    if mut == "z_shift":
        return case.N > 1
    if mut == "unmask":
        return case.masked
    if mut == "swap_Y":
        return case.nD > 1
    return True


@functools.lru_cache(maxsize=None)
def element_eval(name, level, pt="base", mut=None):
    """Everything the element kernels compute at one point, in the broken basis: Dz, the oracle's F and slack, the per-node
    terms of f0, ret_a = sum_k D_k' Y_k (nu x n) and the element blocks Hel_ab (N x p x p), with sum |terms|, smallest term and
    term count.  mut: one deliberate error (MUTATIONS), for tests/test_elem_cases.py."""
    from oracle import mgb_oracle as O
    b = built(name)
    case = b.case
    n, N, p, nu, nD = case.n, case.N, case.p, case.nu, case.nD
    D = list(b.D)
    if mut == "op_shift":
        D = [Dk if nm == "id" else np.roll(Dk, 1, axis=0) for Dk, (_, nm) in zip(D, case.D_full)]
    Dz = dz_at(b, level, pt)
    if mut in ("op_shift", "z_shift"):
        z = b.z0 + b.R[level] @ point(b, level, pt)
        for k, Dk in enumerate(D):
            zk = z[b.state[k] * n:(b.state[k] + 1) * n].reshape(N, p)
            if mut == "z_shift":
                zk = np.roll(zk, 1, axis=0)
            Dz[:, k] = np.einsum("erc,ec->er", Dk, zk).reshape(n)
    bw = b.bw
    if mut == "unmask":
        bw = np.where(bw == 0, np.roll(bw, 1) + np.roll(bw, 2), bw)
    B = O.Barrier(b.Qo, bw)
    with np.errstate(all="ignore"):
        F = O.node_eval(b.Qo, Dz, 0)
        G = B._scale(n, O.node_eval(b.Qo, Dz, 1))
        H = B._scale(n, O.node_eval(b.Qo, Dz, 2))
        f0_terms = B._scale(n, F) + b.w * np.sum(b.c * Dz, axis=1)
    Y = G + b.w[:, None] * b.c
    slack = O.convex_slack(b.Q, Dz[:, :len(case.D_spec)]) if not case.phase1 else None
    mult = np.ones((N, p, nD))
    if mut == "drop_last_node":
        mult[:, p - 1, :] = 0.0
    if mut in ("drop_term", "double_term"):
        k0 = max((k for k in range(nD) if np.any(Y[:, k] != 0) and np.any(H[:, k, k] != 0)), default=0)
        r0 = next(r for r in range(p) if not empty_row((N - 1) * p + r) or p == 1)      # a node whose row of R is not empty
        mult[N - 1, r0, k0] = 0.0 if mut == "drop_term" else 2.0
    YE = Y.reshape(N, p, nD) * mult
    HE = H.reshape(N, p, nD, nD) * mult[:, :, :, None]
    if mut == "swap_Y":
        act = [k for k in range(nD) if np.any(HE[:, :, k, :] != 0)] or [0, nD - 1]
        k1, k2 = act[0], act[-1] if len(act) > 1 else (act[0] + 1) % nD
        perm = list(range(nD))
        perm[k1], perm[k2] = perm[k2], perm[k1]
        YE = YE[:, :, perm]
        HE = HE[:, :, perm][:, :, :, perm]
    old_err = np.seterr(all="ignore")            # masked nodes outside the cone carry NaN * 0 through the term tables
    ret = np.zeros((nu, N, p))
    ret_abs, ret_min = np.zeros((nu, N, p)), np.full((nu, N, p), np.inf)
    for a in range(nu):
        acc = _x(np.zeros((N, p)))
        for k in range(nD):
            if b.state[k] != a:
                continue
            acc = acc + np.einsum("eri,er->ei", _x(D[k]), _x(YE[:, :, k]))
            T = np.abs(D[k]) * np.abs(YE[:, :, k])[:, :, None]            # [e, rr, i]
            ret_abs[a] += T.sum(axis=1)
            ret_min[a] = np.minimum(ret_min[a], np.where(T > 0, T, np.inf).min(axis=1))
        ret[a] = _f(acc)
    blocks = {}
    for a in range(nu):
        for c2 in range(a, nu):
            acc = _x(np.zeros((N, p, p)))
            ab, mn, cnt = np.zeros((N, p, p)), np.full((N, p, p), np.inf), np.zeros((N, p, p))
            for k in range(nD):
                if b.state[k] != a:
                    continue
                for k2 in range(nD):
                    if b.state[k2] != c2 or not np.any(HE[:, :, k, k2]):
                        continue
                    acc = acc + np.einsum("eri,er,erj->eij", _x(D[k]), _x(HE[:, :, k, k2]), _x(D[k2]))
                    T = np.abs(D[k])[:, :, :, None] * np.abs(HE[:, :, k, k2])[:, :, None, None] * np.abs(D[k2])[:, :, None, :]
                    ab += T.sum(axis=1)
                    cnt += (T > 0).sum(axis=1)
                    mn = np.minimum(mn, np.where(T > 0, T, np.inf).min(axis=1))
            blocks[(a, c2)] = (_f(acc), ab, mn, cnt)
    np.seterr(**old_err)
    return dict(Dz=Dz, F=F, slack=slack, f0_terms=f0_terms, ret=ret, ret_abs=ret_abs, ret_min=ret_min, blocks=blocks)


def never_nodes(case):
    """Broken nodes that may not miss the sensitivity condition: the first and last element of every workgroup (both
    workgroup sizes of the wide path) and local node p - 1 of every element."""
    p, N = case.p, case.N
    G = elem_group(p)
    mask = np.zeros((N, p), dtype=bool)
    mask[:, p - 1] = True
    for threads in (128, 256):
        epb = threads // G
        for e0 in range(0, N, epb):
            mask[e0] = True
            mask[min(e0 + epb, N) - 1] = True
    return mask.reshape(-1)


def f0_reference(name, level, pt="base"):
    """(f0, sum |term|): math.fsum of the per-node terms."""
    t = element_eval(name, level, pt)["f0_terms"]
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


def _fine_bound(case):
    return ((case.p + case.nD + 2) * (U53 + UREF) + KERNEL_RTOL) * (1.0 + 2.0 ** -40)


@functools.lru_cache(maxsize=None)
def f1_reference(name, level, pt="base", mut=None):
    b = built(name)
    case = b.case
    n, nu = case.n, case.nu
    ev = element_eval(name, level, pt, mut)
    ret, ab, mn = (ev[k].reshape(nu * n) for k in ("ret", "ret_abs", "ret_min"))
    bound = _fine_bound(case) * ab
    nv = np.tile(never_nodes(case), nu)
    if level == 1:
        rows = np.flatnonzero(b.sel >= 0)
        order = np.argsort(b.sel[rows])
        rows = rows[order]
        return Reference(ret[rows], bound[rows], ab[rows], mn[rows], nv[rows])
    R = np.asarray(b.R[level].todense())
    Ra = np.abs(R)
    val = _f(_x(R.T) @ _x(ret))
    ln = np.count_nonzero(R, axis=0)
    a2 = Ra.T @ np.abs(ret)
    bnd = (Ra.T @ bound + ((ln + 2) * (U53 + UREF) + KERNEL_RTOL) * a2) * (1.0 + 2.0 ** -40)
    pr = Ra * mn[:, None]
    mn2 = np.where(pr > 0, pr, np.inf).min(axis=0)
    return Reference(val, bnd, Ra.T @ ab, mn2, np.zeros(val.shape, dtype=bool))


@functools.lru_cache(maxsize=None)
def f2_reference(name, level, pt="base", mut=None):
    b = built(name)
    case = b.case
    n, nu, N, p = case.n, case.nu, case.N, case.p
    ev = element_eval(name, level, pt, mut)
    nn = nu * n
    e, i, j = np.meshgrid(np.arange(N), np.arange(p), np.arange(p), indexing="ij")
    ra, rb, val, ab, mn, bd = [], [], [], [], [], []
    for (a, c2), (v, s_, m_, cnt) in ev["blocks"].items():
        r1, r2 = (a * n + e * p + i).reshape(-1), (c2 * n + e * p + j).reshape(-1)
        bnd = (((cnt + 3) * (U53 + UREF) + KERNEL_RTOL) * s_ * (1.0 + 2.0 ** -40)).reshape(-1)
        parts = [(r1, r2)] if a == c2 else [(r1, r2), (r2, r1)]
        for x1, x2 in parts:
            ra.append(x1); rb.append(x2); val.append(v.reshape(-1)); ab.append(s_.reshape(-1)); mn.append(m_.reshape(-1)); bd.append(bnd)
    ra, rb, val, ab, mn, bd = (np.concatenate(x) for x in (ra, rb, val, ab, mn, bd))
    nvn = np.tile(never_nodes(case), nu)
    if level == 1:
        m = int(b.sel.max()) + 1
        keep = (b.sel[ra] >= 0) & (b.sel[rb] >= 0)
        ci, cj = b.sel[ra[keep]], b.sel[rb[keep]]
        out = [np.zeros((m, m)) for _ in range(4)]             # value, bound, sum |terms|, smallest term
        out[3][:] = np.inf
        for o, src in zip(out, (val, bd, ab, mn)):
            o[ci, cj] = src[keep]
        nv = np.zeros((m, m), dtype=bool)
        nv[ci, cj] = nvn[ra[keep]] | nvn[rb[keep]]
        return Reference(out[0], out[1], out[2], out[3], nv)
    R = np.asarray(b.R[level].todense())
    Ra = np.abs(R)
    m = R.shape[1]
    live = ab > 0
    ra, rb, val, ab, mn, bd = (x[live] for x in (ra, rb, val, ab, mn, bd))
    Hx = sp.csr_matrix((val, (ra, rb)), shape=(nn, nn))
    V = _f(_x(R.T) @ _x(np.asarray(Hx.todense())) @ _x(R)) if nn <= 600 else np.asarray(R.T @ (Hx @ R))
    A2 = np.zeros((m, m)); Bp = np.zeros((m, m)); Mn = np.full((m, m), np.inf); T = np.zeros((m, m))
    for ci in range(m):
        li = Ra[ra, ci]
        if not li.any():
            continue
        for cj in range(m):
            lj = Ra[rb, cj]
            t = li * np.abs(val) * lj
            nz = t > 0
            if not nz.any():
                continue
            A2[ci, cj] = t.sum()
            T[ci, cj] = nz.sum()
            Mn[ci, cj] = t[nz].min()
            Bp[ci, cj] = (li * bd * lj).sum()
    bound = (Bp + ((T + 2) * (U53 + UREF) + KERNEL_RTOL) * A2) * (1.0 + 2.0 ** -40)
    return Reference(V, bound, A2, Mn, np.zeros((m, m), dtype=bool))
