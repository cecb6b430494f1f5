"""Hand-built problems that hold every evaluation of the node barrier in csrc/cone.hpp (`ep_identity_eval`, `piece_accumulate`,
`wide_piece`, `cone_slack`; DESIGN.md "Cone wall") to a 50-digit reference next to the cone wall, where the residual
r = s^(2/p) - |q|^2 is a difference of nearly equal numbers and every gradient / Hessian entry carries 1/r or 1/r^2.

Layout.  Built like elem_cases.built (plain dataclasses, nothing of the setup layer), with three differences.  (1) Every operator
block is the identity or a DIAGONAL block of powers of two, 2^((e + 2 r + j) % 3 - 1 + shift) for element e, local node r,
operator d_j: the blocks differ per element, D z stays exact, and every term of an f1 / f2 entry belongs to one node, so a
near-wall node cannot swamp an interior neighbour inside a sum.  (2) Only the finest level is evaluated; it is the identity for
every state (level 0 is a pair aggregation that exists only because a problem has levels).  z0 = 0, so z0 + R s = s exactly.
(3) q is data of at most 20 significant bits (u = a 10-bit number times 2^E; with A, b: small integers over powers of two, so
A y + b is exact); s is a full-precision fp64 number tuned in mpmath so that r / s^a = +-2^-k (a = 2/p), then rounded once: the
reference is evaluated at the fp64 point, whatever its exact distance.

Grid.  Nodes are assigned round-robin: k = GRID_K[i % 6], magnitude s ~ 2^e with e = GRID_E[(i // 6) % 6], and in the cases with a
per-node p grid p = GRID_P[(i // 36) % 6]; the other cases take one p each, all six occur.  The number of q components (1 .. 4)
comes from the case.  Exceptions, because one box (b, R) serves all nodes of a phase-I problem and a linear row needs A y + b
exact: the phase-I cases keep s between 2^-12 and R = 2^10 and spend a quarter of their nodes each on the cone wall, the wall of
the slack box (u = +-b (1 - 2^-k)) and the wall of the state box (y_i = +-R (1 - 2^-k)); the two-piece case takes e from
(-100, -20, -8, 24, 40, 100), where the piece with p = 2 is near the wall for e < 0 and the one with p = 4 for e > 0.

With A the s row is a_ss y_s with a_ss a power of two; in the wide case with A it also reads the q columns (a_sc = +-1/16) at the
nodes of magnitude e = 0, 3 where a_ss y_s + sum a_sc y_c is still exact, so that the rank-two term v a_s' + a_s v' of wide_piece
has both halves.  Cases, plans and claims are elem_cases.Case / restated_plan / check_claims; elem_cases' f1_reference and
f2_reference carry the KERNEL_RTOL floor and the sensitivity rule for dropped terms, which do not belong here, so the references
below are formed per node (every operator is diagonal) instead.

A node is DECIDABLE when |r| >= 64 x the bound on the error of the computed r (below); k is lowered (40 -> 32 -> ..) where it is
not, and built() asserts, before it returns a problem, that every active piece of every node of every point is decidable (the
claimed plans are asserted at import; the points are built on first use, like elem_cases.built, to keep collection quick).

Points.  "base"; "trial" = the once-rounded x - TRIAL_STEP dir, tuned with the k grid shifted by one; "outside" = base with a
handful of nodes at r / s^a = -2^-k, k in OUT_K (node_barrier and f0 must be +inf there, a trial landing there finite == 0).

Reference.  Per node F, g, H and the slack from the closed formulas in mpmath at 50 digits on the exact fp64 inputs (checked
against mp.diff of the barrier's definition in test_wall_cases.py); the sums around them (1/n, w c, operator entries) in mpmath too.

Bounds (u = 2^-53).  For a piece with exact a = s^alpha, Q = |q|^2, r = a - Q:
    kappa = (a (1 + |alpha ln s|) + Q) / |r|,        err(r) <= ((2 + 4 |alpha ln s|) a + (nq + 1) Q + |r|) u.
Operation count for err(r): ls = log(s) 1 ulp, i.e. |ls| u, which exp turns into |alpha ls| a u; alpha = fl(2/p) another
|alpha ls| a u; the product alpha * ls a third; exp itself 1 ulp = a u (x 2 for the half-ulp slop of a 1-ulp routine: 2 a u and
a fourth |alpha ls| a u); nq squares and nq - 1 additions (nq + 1) Q u; the subtraction |r| u.  Hence err(r) / |r| <= 4 kappa u + u.
    g term (2 q_i / r, alpha s^(alpha-1) / r, mu / s):      1/r carries 4 kappa u + u, the division and the power s^(alpha-1)
        (own exp/log pair in piece_accumulate and wide_piece: 4 |alpha ln s| u + 2 u <= 4 kappa u; one division in
        ep_identity_eval) and <= 4 products:  <= (8 kappa + 8) u <= 16 kappa u |term|     (kappa >= 1)
    H term (4 q_i q_j / r^2, 2 / r, coef_qs q_i, the three terms of H_ss):  1/r^2 doubles the first part, the powers
        s^(alpha-2), s^(2 alpha-2) cost <= 8 kappa u:  <= (16 kappa + 12) u <= 32 kappa u |term|
    F = -log r - mu log s:  (16 kappa + 2 |ln r| + 3 mu |ln s|) u, absolute
    slack = -min(s - |q|^p, s):  16 ((1 + |p/2 ln Q|) |q|^p + |s|) u
    LINEAR rows and box terms (arguments exact):  16 u |term|
An entry of g, H in the y layout (A' g_z, A' H_z A, the scatter of several pieces, box terms), of f1 or of f2 gets the sum of its
terms' bounds plus (T + 3) u sum |terms|, as in elem_cases: T is the number of terms of the entry (one product chain each), and
the sum part is applied once, at the outermost entry (an f1 / f2 entry takes only the terms' own bounds up from the node level).  The wide path's algebra (projector + rank two)
forms the same sums with |v| = |A_q' q| <= sum |A| |q|, so the term-wise bound covers it.  No KERNEL_RTOL floor is added, and no
entry is skipped.  No constant here was tuned from a device observation."""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import mpmath as mp
import numpy as np
import scipy.sparse as sp

import elem_cases as E
from dense_cases import rnd, sign
from gate_cases import U53, weight

DPS = 50
GRID_K = (1, 8, 16, 24, 32, 40)
GRID_P = (1.0, 1.5, 2.0, 3.0, 4.0, 16.0)
GRID_E = (-100, -20, 0, 3, 20, 100)
GRID_E_TWO_PIECE = (-100, -20, -8, 24, 40, 100)
OUT_K = (8, 24, 40)
DECIDABLE = 64
ORACLE_SHARE = 0.25
TRIAL_STEP = E.TRIAL_STEP
BOX = (2.0 ** 4, 2.0 ** 10)                      # (b, R) of the phase-I cases
EP, LIN = E.KIND_EP, E.KIND_LINEAR
C_G, C_H, C_LIN = 16, 32, 16
GRID_P_ARR = np.array(GRID_P)


@dataclass
class Case(E.Case):
    pvals: tuple = ()                  # per EP piece: a constant p, or "grid"
    shift: int = 0                     # exponent offset of the non-identity operator blocks
    dense: bool = False                # p > 64: the dense node kernels (csrc/dense.hip)


_c = E._claims
CASES = [
    # 1. ep_identity_eval in the fast kernels, default signature: the bench's family (4, 7) and (3, 2) with one q component
    Case("wall_p7", 7, 33, E._D4, E._P4, _c(("fast_default", 4, 7), ("generic", 4, 0), 8, 32, 2, 2), pvals=(1.5,)),
    Case("wall_p2", 2, 129, E._D3, E._P3, _c(("fast_default", 3, 2), ("generic", 3, 0), 2, 128, 2, 1), pvals=(3.0,)),
    # 2. ep_identity_eval in elem_kernel<5>: (5, 3) is not in the fast table; three q components
    Case("wall_generic", 3, 65, E._D5, E._P5, _c(("generic", 5, 0), ("generic", 5, 0), 4, 64, 2, 3), pvals=(4.0,)),
    # 3. ep_identity_eval in the dense node kernels: one element of 65 nodes, per-node p
    Case("wall_dense", 65, 1, E._D3, E._P3, dict(dense=True), pvals=("grid",), dense=True),
    # 4. piece_accumulate on a fast instantiation: non-identity A, b, per-node p
    Case("wall_p7_A", 7, 33, E._D4, [(EP, (1, 2, 3), "A")], _c(("fast_default", 4, 7), ("generic", 4, 0), 8, 32, 2, 2), pvals=("grid",)),
    # 5. piece_accumulate under phase I: cobarrier with slack_pos, runtime signature, box terms at their own wall
    Case("wall_p7_phase1", 7, 33, E._D4, E._P4, _c(("fast_runtime", 7, 7), ("generic", 7, 0), 8, 32, 2, 2), phase1=True,
         pvals=("grid",), shift=-4),
    # 6. two EP pieces with a select mask and one LINEAR piece, elem_kernel<9>
    Case("wall_two_piece", 3, 65, E._D9, [(EP, (1, 2, 3, 8), ""), (EP, (4, 5, 8), ""), (LIN, (6, 7, 0), "")],
         _c(("generic", 9, 0), ("generic", 9, 0), 4, 64, 2, 3), select=True, pvals=(2.0, 4.0)),
    # 7. wide_piece: identity A, the gram loop, the phase-I image, and dense_node_wide_kernel
    Case("wall_wide", 4, 65, E._W7, [(EP, E._PW7, "")], _c(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3), pvals=(1.0,)),
    Case("wall_wide_A", 4, 65, E._W7, [(EP, E._PW7, "A")], _c(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3),
         pvals=("grid",)),
    Case("wall_wide_phase1", 4, 65, E._W7, [(EP, E._PW7, "")], _c(("wide", 0, 0), ("wide", 0, 0), 4, 64, 2, 2, f2_EPB=32, f2_grid=3),
         phase1=True, pvals=("grid",), shift=-5),
    Case("wall_dense_wide", 65, 1, E._W7, [(EP, E._PW7, "")], dict(dense=True), pvals=(16.0,), dense=True),
]
CASE = {c.name: c for c in CASES}
NAMES = [c.name for c in CASES]
POINTS = ("base", "trial", "outside")


def expected_plan(name, mode):
    """What DeviceProblem.elem_plan(mode) must report: the dense kind for p > 64, elem_cases' restated gate arithmetic otherwise."""
    case = CASE[name]
    return dict(kind="dense") if case.dense else E.restated_plan(case, mode)


def check_claims(case):
    if case.dense:
        return case.p > 64 and case.N == 1
    return E.check_claims(case)


for _case in CASES:
    assert check_claims(_case), _case.name
assert {pv for c in CASES for pv in c.pvals if pv != "grid"} == set(GRID_P)            # every p as a constant of some case
assert {len(idx) - 1 for c in CASES for kd, idx, _ in c.pieces if kd == EP} >= {1, 2, 3}


# ---------------------------------------------------------------------------------------------------------------------
# exact helpers
# ---------------------------------------------------------------------------------------------------------------------

def _mpf(v):
    return mp.mpf(float(v))


def _exact_sum(*vals):
    """The fp64 numbers add up to an fp64 number: True, and the number."""
    t = sum(Fraction(float(v)) for v in vals)
    return Fraction(float(t)) == t, float(t)


def significant_bits(v):
    """Number of significant bits of the fp64 number v."""
    if v == 0:
        return 0
    m = Fraction(abs(float(v)))
    num, den = m.numerator, m.denominator
    while num % 2 == 0:
        num //= 2
    while den % 2 == 0:
        den //= 2
    assert den == 1
    return num.bit_length()


def ep_measure(q, s, p):
    """(r, a, kappa, err(r)) of one power-cone point, in mpmath: q, s, p exact fp64 inputs (s: mpf, may be an exact sum)."""
    al = 2 / _mpf(p)
    ls = mp.log(s)
    a = mp.exp(al * ls)
    Q = sum((_mpf(x) ** 2 for x in q), mp.mpf(0))
    r = a - Q
    t = abs(al * ls)
    return r, a, (a * (1 + t) + Q) / abs(r), ((2 + 4 * t) * a + (len(q) + 1) * Q + abs(r)) * U53


def decidable(q, s, p):
    r, _, _, err = ep_measure(q, s, p)
    return abs(r) >= DECIDABLE * err


def tune_s(q, p, k, sigma=1):
    """The fp64 s with s^(2/p) - |q|^2 = sigma 2^-k s^(2/p) before rounding; k is lowered along GRID_K until the rounded
    point is decidable.  Returns (s, k)."""
    Q = sum((_mpf(x) ** 2 for x in q), mp.mpf(0))
    ks = [kk for kk in sorted(set(GRID_K + OUT_K)) if kk <= k]
    while ks:
        kk = ks.pop()
        s = float((Q / (1 - sigma * mp.mpf(2) ** -kk)) ** (_mpf(p) / 2))
        if decidable(q, _mpf(s), p):
            return s, kk
    raise AssertionError(("no decidable k", q, p, k))


# ---------------------------------------------------------------------------------------------------------------------
# the problems
# ---------------------------------------------------------------------------------------------------------------------

def operator_diag(name, case):
    """The diagonal (n,) of an operator: powers of two that differ per element and local node."""
    nodes = np.arange(case.n)
    if name == "id":
        return np.ones(case.n)
    j = int(name[1:])
    return 2.0 ** ((nodes // case.p + 2 * (nodes % case.p) + j) % 3 - 1 + case.shift)


@dataclass
class Built:
    case: Case
    D: list                            # nD diagonals (n,)
    state: list
    R: list
    pts: dict                          # point name -> the finest level's vector (= z, z0 is 0)
    dirs: dict                         # "trial" / "outside": the direction with pts[.] = fl(base - TRIAL_STEP dir)
    knode: dict                        # point name -> (n,) the largest k = -log2 |r / s^a| of the node's active pieces at the point
    out_nodes: np.ndarray              # the nodes outside the cone at the point "outside"
    z0: np.ndarray
    w: np.ndarray
    c: np.ndarray
    box: tuple
    M: object = field(repr=False, default=None)
    Q: object = field(repr=False, default=None)
    Qo: object = field(repr=False, default=None)


def _flat(A):
    """(n, nr, nc) [r, c] -> the column-major flattened per-node grid of Piece.A."""
    n = A.shape[0]
    return A.transpose(0, 2, 1).reshape(n, -1)


@dataclass
class _Layout:
    """What a case assigns to its nodes before any tuning: the grid, the operators, the EP pieces' grids and the states u."""
    case: Case
    D: list                            # nD diagonals (n,)
    state: list
    kgrid: np.ndarray
    egrid: np.ndarray
    cls: np.ndarray                    # phase I: 0 cone wall, 1 slack box, 2 state box (u), 3 state box (s); else 0
    p0: np.ndarray                     # the p that decides the node's magnitude
    ep: list                           # [(piece index, idx, options)] of the EP pieces
    grids: dict                        # piece index -> (A (n, ni, ni) [r, c], b (n, ni), p (n,), mu (n,))
    U: np.ndarray                      # (nu, n): the u states; the slack rows are filled by tuned_point
    sel: object

    def active(self, i, j):
        return self.sel is None or self.sel[i, j] != 0

    def rows(self, Ux):
        return np.stack([self.D[k] * Ux[self.state[k]] for k in range(len(self.D))], axis=1)

    def q_at(self, j, i, Dz_i):
        """The q part of A y[idx] + b of EP piece j at node i: fp64 numbers, every product and the sum asserted exact."""
        A, b_, _, _ = self.grids[j]
        idx = self.case.pieces[j][1]
        ni = len(idx)
        yq = [Dz_i[idx[cc]] for cc in range(ni - 1)]
        q = []
        for r in range(ni - 1):
            ok, v = _exact_sum(*[A[i, r, cc] * yq[cc] for cc in range(ni - 1)], b_[i, r])
            assert ok and all(Fraction(float(A[i, r, cc] * yq[cc])) == Fraction(float(A[i, r, cc])) * Fraction(float(yq[cc]))
                              for cc in range(ni - 1)), (self.case.name, i, r)
            q.append(v)
        return q


def _piece_grids(case, j, idx, opt, nodes, Eu):
    """A (n, ni, ni) as [r, c], b (n, ni), p (n,) of the EP piece j."""
    n, ni = nodes.size, len(idx)
    A = np.broadcast_to(np.eye(ni), (n, ni, ni)).copy()
    b = np.zeros((n, ni))
    if "A" in opt:
        for r in range(ni - 1):
            for cc in range(ni - 1):
                if r != cc:          # couplings among the q columns: +-1/4 (narrow) or +-1/8 (wide), diagonally dominant
                    A[:, r, cc] = sign(nodes + 3 * r, 0.5 + cc) * (0.25 if ni <= 4 else 0.125) * (1 + (nodes + r + cc) % 2 * (ni <= 3))
            b[:, r] = sign(nodes, 2.1 + r) * (1 + (nodes + r) % 3) / 4 * 2.0 ** Eu
        A[:, ni - 1, ni - 1] = np.array([0.5, 2.0, 1.0])[nodes % 3]
    pv = case.pvals[j]
    p = GRID_P_ARR[(nodes // 36) % 6] if pv == "grid" else np.full(n, float(pv))
    return A, b, p


def _layout(case):
    p, n, nu, nD, nu0 = case.p, case.n, case.nu, case.nD, case.nu0
    nodes = np.arange(n)
    D = [operator_diag(nm, case) for _, nm in case.D_full]
    state = [a for a, _ in case.D_full]
    ep = [(j, idx, opt) for j, (kd, idx, opt) in enumerate(case.pieces) if kd == EP]
    two_piece = len(ep) > 1
    RR = BOX[1]
    if case.phase1:
        cls = nodes % 4
        kgrid = np.array(GRID_K)[(nodes // 4) % 6]
        egrid = np.array([-12, -4, 0, 3, -8, 1])[(nodes // 24) % 6]
        p0 = np.where(cls >= 2, 1.0, GRID_P_ARR[(nodes // 8) % 6])           # a state at the wall of its box fits the cone only at p = 1
    else:
        cls = np.zeros(n, dtype=np.int64)
        kgrid = np.array(GRID_K)[nodes % 6]
        egrid = np.array(GRID_E_TWO_PIECE if two_piece else GRID_E)[(nodes // 6) % 6]
        p0 = np.full(n, float(case.pvals[0])) if case.pvals[0] != "grid" else GRID_P_ARR[(nodes // 36) % 6]
        if two_piece:                # p = 2 decides the magnitude for e < 0 and p = 4 for e > 0
            p0 = np.where(egrid < 0, 2.0, 4.0)
    # the exponent of u: |q|^2 ~ s^(2/p) with s ~ 2^e  <=>  u ~ 2^(e / p)
    Eu = np.rint(egrid / p0).astype(np.int64)
    grids = {}
    for j, idx, opt in ep:
        A, b_, pj = _piece_grids(case, j, idx, opt, nodes, Eu)
        if case.phase1:
            pj = p0
        grids[j] = (A, b_, pj, np.where(pj < 2, 1.0, 2.0))
    # states: u = 10-bit data x 2^Eu; phase I, class 2: u at the wall of the state box, alternating sides
    U = np.zeros((nu, n))
    for a in range(nu0 - 1):
        U[a] = sign(nodes % p + a, 1.3) * rnd(weight(3 * nodes + 40 * a, 1 + a)) * 2.0 ** Eu
        if case.phase1:
            U[a] = np.where(cls == 2, sign(nodes + a, 0.4) * RR * (1 - 2.0 ** -kgrid), U[a])
    sel = None
    if case.select:
        sel = np.ones((n, len(case.pieces)))
        for kk in range(len(case.pieces)):
            sel[nodes % (5 + kk) == 3, kk] = 0.0
    return _Layout(case, D, state, kgrid, egrid, cls, p0, ep, grids, U, sel)


def _phase1_node(L, i, jt, q, k_i, sigma):
    """(y_s, slack, k) of node i of a phase-I case, by its class; y_s + slack is an fp64 number."""
    name, (bb, RR) = L.case.name, BOX
    cl = L.cls[i]
    if cl == 0:                      # the cone wall: s = y_s + slack, 0 < slack < s, a multiple of the spacing of s
        s_t, k_i = tune_s(q, L.grids[jt][2][i], k_i, sigma)
        ex = math.frexp(s_t)[1] - 1
        slack = 2.0 ** (min(ex, 3) - 1) * (1 + (i % 4) / 4)
        ok, ys = _exact_sum(s_t, -slack)
        assert ok and _exact_sum(ys, slack) == (True, s_t), (name, i)
        return ys, slack
    if cl == 1:                      # the phase-I slack at the wall of its box; the cone well inside
        slack = float(sign(i, 0.9)) * bb * (1 - 2.0 ** -k_i)
        S = 32.0 + math.ceil(8.0 * max(math.sqrt(sum(x * x for x in q)), 1.0) ** L.grids[jt][2][i])
        ok, ys = _exact_sum(S, -slack)
        assert ok and _exact_sum(ys, slack) == (True, S) and abs(ys) < RR, (name, i)
        return ys, slack
    if cl == 2:                      # u at the wall of the state box (set by _layout); s = R / 2 + 2
        return RR / 2, 2.0
    return RR * (1 - 2.0 ** -k_i), 2.0 + i % 3          # y_s at the wall of the state box


def tuned_point(L, kshift, outside_nodes=(), bad=None):
    """The states (nu, n) with every node's s tuned to its k (the grid shifted by kshift; the nodes of outside_nodes to -2^-k).
    bad: a set that collects the nodes whose s row a_ss y_s + sum_c a_sc y_c is not exact (None: assert that there is none)."""
    case = L.case
    nu0 = case.nu0
    s_state = nu0 - 1
    Ux = L.U.copy()
    Dz = L.rows(Ux)
    out_k = {int(i): OUT_K[t % len(OUT_K)] for t, i in enumerate(outside_nodes)}
    for i in range(case.n):
        k_i = int(GRID_K[(GRID_K.index(int(L.kgrid[i])) + kshift) % 6])
        sigma = 1
        if i in out_k:
            k_i, sigma = out_k[i], -1
        # the piece that is tuned: the active EP piece whose p decides the node's magnitude, else any active one
        jt = next((j for j, _, _ in L.ep if L.active(i, j) and L.grids[j][2][i] == L.p0[i]), None)
        if jt is None:
            jt = next((j for j, _, _ in L.ep if L.active(i, j)), None)
        if jt is None:               # every power cone deselected: s is free
            Ux[s_state, i] = 2.0 ** int(L.egrid[i])
            continue
        q = L.q_at(jt, i, Dz[i])
        if case.phase1:
            Ux[s_state, i], Ux[nu0, i] = _phase1_node(L, i, jt, q, k_i, sigma)
            continue
        # s = a_ss y_s + sum_c a_sc y_c, exact
        s_t, _ = tune_s(q, L.grids[jt][2][i], k_i, sigma)
        A = L.grids[jt][0]
        ass, idx_t = A[i, -1, -1], case.pieces[jt][1]
        ok, rest = _exact_sum(*[A[i, -1, cc] * Dz[i, idx_t[cc]] for cc in range(len(idx_t) - 1)])
        ok2, num = _exact_sum(s_t, -rest)
        ys = num / ass
        if not (ok and ok2 and _exact_sum(rest, ass * ys) == (True, s_t) and 0 < num <= s_t):
            assert bad is not None, (case.name, i)
            bad.add(i)
            ys = s_t / ass
        Ux[s_state, i] = ys
    return Ux


def _outside_nodes(L):
    """The first node of the second workgroup, the last node and a few between (phase I: among the cone-wall nodes), each with an
    active power cone."""
    case, n = L.case, L.case.n
    out = np.array(sorted({1, n // 3, n // 2 + 1, n - 2, (256 // E.elem_group(case.p)) * case.p % n, n - 1}), dtype=np.int64)
    if case.phase1:
        out = np.flatnonzero(L.cls == 0)[[0, 3, 7, -1]]
    return np.array([int(v) for v in out if any(L.active(v, j) for j, _, _ in L.ep)], dtype=np.int64)


def _wide_s_row(L, out_nodes):
    """The s row of a wide piece with A also reads the q columns (a_sc = +-1/16) at the nodes of magnitude e = 0, 3 where that
    keeps s exact at all three points: set everywhere there, then cleared at the nodes a first tuning pass reports."""
    for j, idx, opt in L.ep:
        if "A" in opt and len(idx) > E.NARROW_W:
            A = L.grids[j][0]
            for cc in range(len(idx) - 1):
                yc = L.D[idx[cc]] * L.U[L.state[idx[cc]]]
                A[:, -1, cc] = np.where(np.isin(L.egrid, (0, 3)), np.sign(yc) / 16, 0.0)
            bad = set()
            for ks, outs in ((0, ()), (1, ()), (0, tuple(out_nodes))):
                tuned_point(L, ks, outs, bad)
            A[sorted(bad), -1, :len(idx) - 1] = 0.0


def _points(L, out_nodes):
    """pts, dirs: base, and the once-rounded steps to the trial point and to the point with out_nodes outside."""
    from test_gpu_elem import exact_step
    case = L.case
    nu, n, nu0 = case.nu, case.n, case.nu0
    s_state = nu0 - 1
    Ub = tuned_point(L, 0)
    base = Ub.reshape(-1)
    pts, dirs = dict(base=base), {}
    for pt, (ks, outs) in dict(trial=(1, ()), outside=(0, tuple(out_nodes))).items():
        Ut = tuned_point(L, ks, outs)
        d = 2.0 * (base - Ut.reshape(-1))
        if case.phase1 and pt == "trial":
            # the sum y_s + slack must stay exact at the rounded trial point: move y_s alone, by a multiple of the coarser spacing
            d = d.reshape(nu, n)
            d[nu0] = 0.0
            for i in range(n):
                ys0, yt, sl = Ub[s_state, i], Ut[s_state, i], Ub[nu0, i]
                quantum = 4.0 * max(np.spacing(abs(ys0) + abs(sl)), np.spacing(abs(yt) + abs(sl)))
                d[s_state, i] = 2.0 * (round((ys0 - yt) / quantum) * quantum)
                if not _exact_sum(exact_step([ys0], [d[s_state, i]], TRIAL_STEP)[0], sl)[0]:
                    d[s_state, i] = 0.0
            d = d.reshape(-1)
        dirs[pt] = d
        pts[pt] = exact_step(base, d, TRIAL_STEP)
    for pt in POINTS:
        assert np.all(np.isfinite(pts[pt])), (case.name, pt)
    return pts, dirs, Ub


def _convex(L, Dzb):
    """The Convex of the case: the EP pieces from their grids; LINEAR rows F_v = A y + b = 2^-k x the magnitude of y, exact
    (A small integers over powers of two, b = 2^-k scale - A y at the base point; its rows read u states only)."""
    from mgb_amd.convex import Convex, Piece
    case, n = L.case, L.case.n
    nodes = np.arange(n)
    pcs = []
    for j, (kd, idx, opt) in enumerate(case.pieces):
        ni = len(idx)
        if kd == EP:
            A, b_, pj, mu = L.grids[j]
            pcs.append(Piece(EP, tuple(idx), _flat(A), b_.copy(), pj.copy(), mu.copy()))
            continue
        r_, c_ = np.arange(ni)[None, :, None], np.arange(ni)[None, None, :]
        Am = sign(nodes[:, None, None] + r_, 0.8 + c_) * np.array([0.5, 1.0, 0.25])[(nodes[:, None, None] + r_ + 2 * c_) % 3]
        yb = Dzb[:, list(idx)]
        bl = np.zeros((n, ni))
        for i in range(n):
            for r in range(ni):
                ok, acc = _exact_sum(*[Am[i, r, cc] * yb[i, cc] for cc in range(ni)])
                kr = GRID_K[(i + r) % 6]
                Fv = 2.0 ** (math.frexp(yb[i, 0])[1] - kr) * (1 + ((i + r) % 4) / 4)
                ok2, bv = _exact_sum(Fv, -acc)
                assert ok and ok2 and _exact_sum(acc, bv) == (True, Fv), (case.name, i, r)
                bl[i, r] = bv
        pcs.append(Piece(LIN, tuple(idx), _flat(Am), bl))
    return Convex(pcs, L.sel)


def _amg(case, w):
    """(R, M): a pair aggregation per state (never evaluated) and the identity; the AMG around diagonal operator blocks."""
    from mgb_amd.blockmatrices import BlockColumn, BlockDiag
    from mgb_amd.multigrid import AMG, Geometry
    p, N, n, nu = case.p, case.N, case.n, case.nu
    nodes = np.arange(n)
    agg = sp.block_diag([sp.csr_matrix((np.ones(n), (nodes, nodes // 2)), shape=(n, (n + 1) // 2)) for _ in range(nu)])
    R = [sp.csr_matrix(agg), sp.identity(nu * n, format="csr")]
    blk = {}
    for nm in sorted({nm for _, nm in case.D_full}):
        data = np.zeros((p, p, N))
        dg = operator_diag(nm, case).reshape(N, p)
        for r in range(p):
            data[r, r, :] = dg[:, r]
        blk[nm] = BlockDiag(data)
    x = np.cos(0.37 * nodes + 0.1).reshape(n, 1)
    geom = Geometry(discretization=None, t=nodes.reshape(N, p).T.copy(), x=x.reshape(N, p, 1).transpose(1, 0, 2).copy(), w=w, operators=blk)
    M = AMG(geometry=geom, x=x.copy(), w=w, R_fine=R, D_fine=[BlockColumn(blk[nm], a, nu) for a, nm in case.D_full],
            state_names=[f"v{a}" for a in range(nu)], D_spec=list(case.D_full))
    return R, M


def _check_points(b, L):
    """The points as they are after rounding: q data of <= 20 bits at the tuned nodes, y_s + slack exact, every active piece
    decidable, outside exactly at out_nodes.  Fills knode: the nearest k of the node's active pieces at the actual point."""
    case = b.case
    for pt in POINTS:
        Dz = dz_at(b, pt)
        b.knode[pt] = np.zeros(case.n, dtype=np.int64)
        for i in range(case.n):
            signs = []
            for j, idx, _ in L.ep:
                if not L.active(i, j):
                    continue
                q = L.q_at(j, i, Dz[i])
                if L.cls[i] == 0:
                    assert all(significant_bits(v) <= 20 for v in q), (case.name, pt, i, q)
                if case.phase1:
                    assert _exact_sum(Dz[i, idx[-1]], Dz[i, case.NC - 1])[0], (case.name, pt, i)
                r, a, _, err = ep_measure(q, _s_of(b, j, i, Dz[i]), L.grids[j][2][i])
                assert abs(r) >= DECIDABLE * err, (case.name, pt, i, j, float(r), float(err))
                signs.append(r > 0)
                b.knode[pt][i] = max(b.knode[pt][i], int(round(-float(mp.log(abs(r) / a, 2)))))
            assert (not all(signs)) == (pt == "outside" and i in b.out_nodes), (case.name, pt, i, signs)


@functools.lru_cache(maxsize=None)
def built(name):
    from oracle import mgb_oracle as O
    mp.mp.dps = DPS
    case = CASE[name]
    n, nu, nD = case.n, case.nu, case.nD
    nodes = np.arange(n)
    L = _layout(case)
    out_nodes = _outside_nodes(L)
    _wide_s_row(L, out_nodes)
    pts, dirs, Ub = _points(L, out_nodes)
    w = np.round(weight(nodes, 2) * E.ONE) / (E.ONE * 256)
    # c: 10-bit data scaled by the magnitude of its row of D z, so that no term of f0 or of Y = g / n + w c drowns the others
    Dzb = L.rows(Ub)
    c = np.stack([sign(nodes, 0.3 + k) * rnd(weight(2 * nodes + k, k + 4)) for k in range(nD)], axis=1)
    c = c * 2.0 ** -np.where(Dzb != 0, np.frexp(Dzb)[1], 0)
    for k in range(nD):
        if L.state[k] in case.slack_states:
            c[:, k] = -np.abs(c[:, k])
    Q = _convex(L, Dzb)
    R, M = _amg(case, w)
    b = Built(case, L.D, L.state, R, pts, dirs, {}, out_nodes, np.zeros(nu * n), w, c, BOX, M, Q,
              O.FeasConvex(Q, BOX[0], BOX[1], case.NC) if case.phase1 else Q)
    _check_points(b, L)
    return b


def _s_of(b, j, i, Dz_i):
    """The exact s of EP piece j at node i (mpf): a_ss y_s (+ the phase-I slack), an fp64 number by construction at base points;
    at a rounded trial point of a phase-I case the exact sum."""
    pc = b.Q.pieces[j]
    ni = pc.ni
    s = sum((_mpf(pc.A[i, (ni - 1) + ni * c]) * _mpf(Dz_i[pc.idx[c]]) for c in range(ni)), mp.mpf(0)) + _mpf(pc.b[i, ni - 1])
    if b.case.phase1:
        s += _mpf(Dz_i[b.case.NC - 1])
    return s


def dz_at(b, pt):
    """D z (n x nD) at a point: diagonal powers of two times fp64 numbers, exact."""
    n = b.case.n
    z = b.pts[pt]
    return np.stack([b.D[k] * z[b.state[k] * n:(b.state[k] + 1) * n] for k in range(len(b.D))], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# the 50-digit reference of one node: closed formulas, values with sum |terms| and bounds
# ---------------------------------------------------------------------------------------------------------------------

class _Acc:
    """An entry as a sum of terms: value, sum |terms|, sum of the terms' own bounds, number of terms."""
    __slots__ = ("v", "a", "b", "t")

    def __init__(self):
        self.v, self.a, self.b, self.t = mp.mpf(0), mp.mpf(0), mp.mpf(0), 0

    def add(self, val, rel):
        if val != 0:
            self.v += val
            self.a += abs(val)
            self.b += abs(val) * rel
            self.t += 1

    def bound(self):
        return self.b + (self.t + 3) * U53 * self.a


def ep_closed(q, s, p, mu):
    """F, the terms of g_z and H_z of -log(s^(2/p) - |q|^2) - mu log s in (q, s), closed formulas in mpmath.
    Returns None outside the cone, else (F, F bound, kappa, gz, Hz): gz[i] / Hz[i][j] lists of terms."""
    nq = len(q)
    al = 2 / p
    ls = mp.log(s)
    a = mp.exp(al * ls)
    Q = sum((x * x for x in q), mp.mpf(0))
    r = a - Q
    if r <= 0:
        return None
    kap = (a * (1 + abs(al * ls)) + Q) / r
    F = -mp.log(r) - mu * ls
    Fb = (16 * kap + 2 * abs(mp.log(r)) + 3 * mu * abs(ls)) * U53
    am1 = a / s
    gz = [[2 * x / r] for x in q] + [[-al * am1 / r, -mu / s]]
    cqs = -2 * al * am1 / r ** 2
    Hz = [[[] for _ in range(nq + 1)] for _ in range(nq + 1)]
    for i in range(nq):
        for j in range(nq):
            Hz[i][j] = [4 * q[i] * q[j] / r ** 2] + ([2 / r] if i == j else [])
        Hz[i][nq] = [cqs * q[i]]
        Hz[nq][i] = [cqs * q[i]]
    Hz[nq][nq] = [-al * (al - 1) * am1 / s / r, al * al * am1 * am1 / r ** 2, mu / s ** 2]
    return F, Fb, kap, gz, Hz


@functools.lru_cache(maxsize=None)
def _node_cached(name, i, row):
    return _node(built(name), i, row)


def _node(b, i, row):
    """The node barrier of case b at node i for the row y = D z (a tuple of fp64 numbers): dict(F, Fb, g, gb, H, Hb, slack, slackb,
    inside); g, H in the y layout as floats with their bounds."""
    case, Q = b.case, b.Q
    nD, NC = case.nD, case.NC
    y = [_mpf(v) for v in row]
    bb, RR = (_mpf(v) for v in b.box)
    extra = y[NC - 1] if case.phase1 else mp.mpf(0)
    G = [_Acc() for _ in range(nD)]
    H = [[_Acc() for _ in range(nD)] for _ in range(nD)]
    Fa = _Acc()
    Fb_own = mp.mpf(0)
    inside = True
    slack, slackb = None, mp.mpf(0)
    for k, pc in enumerate(Q.pieces):
        if Q.select is not None and Q.select[i, k] == 0:
            continue
        ni, idx = pc.ni, pc.idx
        if pc.kind == EP:
            A = [[_mpf(pc.A[i, r + ni * c]) for c in range(ni)] for r in range(ni)]
            z = [sum((A[r][c] * y[idx[c]] for c in range(ni)), mp.mpf(0)) + _mpf(pc.b[i, r]) for r in range(ni)]
            p0, mu = _mpf(pc.p[i]), _mpf(pc.mu[i])
            q, s0 = z[:ni - 1], z[ni - 1]
            Qn = sum((x * x for x in q), mp.mpf(0))
            qp = Qn ** (p0 / 2)
            val = -min(s0 - qp, s0)
            vb = 16 * ((1 + abs(p0 / 2 * mp.log(Qn))) * qp + abs(s0)) * U53
            if slack is None or val > slack:
                slack = val
            slackb = max(slackb, vb)
            res = ep_closed(q, s0 + extra, p0, mu)
            if res is None:
                inside = False
                continue
            F, Fb, kap, gz, Hz = res
            Fa.add(F, 0)
            Fb_own += Fb
            cols = list(range(ni))
            Ax = [row_[:] for row_ in A]
            names_ = list(idx)
            if case.phase1:          # the cobarrier: the slack column is a copy of the s row's unit vector
                for r in range(ni):
                    Ax[r].append(mp.mpf(1) if r == ni - 1 else mp.mpf(0))
                names_.append(NC - 1)
            for c, kc in enumerate(names_):
                for r in range(ni):
                    for t in gz[r]:
                        G[kc].add(Ax[r][c] * t, C_G * kap * U53)
                for c2, kc2 in enumerate(names_):
                    for r in range(ni):
                        if Ax[r][c] == 0:
                            continue
                        for r2 in range(ni):
                            if Ax[r2][c2] == 0:
                                continue
                            for t in Hz[r][r2]:
                                H[kc][kc2].add(Ax[r][c] * t * Ax[r2][c2], C_H * kap * U53)
        else:
            nc = pc.nc
            A = [[_mpf(pc.A[i, r + nc * c]) for c in range(ni)] for r in range(nc)]
            Fv = [sum((A[r][c] * y[idx[c]] for c in range(ni)), mp.mpf(0)) + _mpf(pc.b[i, r]) + extra for r in range(nc)]
            val = -(min(Fv) - extra)
            if slack is None or val > slack:
                slack = val
            slackb = max(slackb, C_LIN * U53 * abs(val))
            if min(Fv) <= 0:
                inside = False
                continue
            names_ = list(idx) + ([NC - 1] if case.phase1 else [])
            for r in range(nc):
                Fa.add(-mp.log(Fv[r]), C_LIN * U53)
                Ar = A[r] + ([mp.mpf(1)] if case.phase1 else [])
                for c, kc in enumerate(names_):
                    G[kc].add(-Ar[c] / Fv[r], C_LIN * U53)
                    for c2, kc2 in enumerate(names_):
                        H[kc][kc2].add(Ar[c] * Ar[c2] / Fv[r] ** 2, C_LIN * U53)
    if case.phase1:
        u = y[NC - 1]
        for lim, ks in ((bb, [NC - 1]), (RR, list(range(NC, nD)))):
            for kk in ks:
                v = y[kk]
                if lim - v <= 0 or lim + v <= 0:
                    inside = False
                    continue
                Fa.add(-mp.log(lim - v), C_LIN * U53)
                Fa.add(-mp.log(lim + v), C_LIN * U53)
                G[kk].add(1 / (lim - v), C_LIN * U53)
                G[kk].add(-1 / (lim + v), C_LIN * U53)
                H[kk][kk].add(1 / (lim - v) ** 2, C_LIN * U53)
                H[kk][kk].add(1 / (lim + v) ** 2, C_LIN * U53)
    out = dict(inside=inside, slack=-mp.inf if slack is None else slack, slackb=slackb)      # every piece deselected: -inf, as the oracle
    if inside:
        out.update(F=Fa.v, Fb=Fb_own + Fa.bound(), G=G, H=H)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the reference of a whole point
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class PointRef:
    Dz: np.ndarray
    inside: np.ndarray
    F: np.ndarray                      # +inf outside
    Fb: np.ndarray
    slack: object
    slackb: object
    f0: float
    f0b: float
    f1: np.ndarray                     # (nu n,), state-major; NaN at nodes outside
    f1b: np.ndarray
    f2: np.ndarray                     # (nu n, nu n)
    f2b: np.ndarray
    knode: np.ndarray


def _f(x):
    return float(x)


@functools.lru_cache(maxsize=None)
def reference(name, pt):
    b = built(name)
    mp.mp.dps = DPS
    case = b.case
    n, nu, nD = case.n, case.nu, case.nD
    Dz = dz_at(b, pt)
    inv_n = mp.mpf(1) / n
    inside = np.ones(n, dtype=bool)
    F, Fb = np.full(n, np.inf), np.zeros(n)
    slack, slackb = np.zeros(n), np.zeros(n)
    f0 = _Acc()
    f0_own = mp.mpf(0)
    f1, f1b = np.full(nu * n, np.nan), np.zeros(nu * n)
    f2, f2b = np.zeros((nu * n, nu * n)), np.zeros((nu * n, nu * n))
    for i in range(n):
        nd = _node_cached(name, i, tuple(float(v) for v in Dz[i]))
        slack[i], slackb[i] = _f(nd["slack"]), _f(nd["slackb"])
        wi = _mpf(b.w[i])
        for k in range(nD):
            f0.add(wi * _mpf(b.c[i, k]) * _mpf(Dz[i, k]), 0)
        if not nd["inside"]:
            inside[i] = False
            continue
        F[i], Fb[i] = _f(nd["F"]), _f(nd["Fb"])
        f0.add(inv_n * nd["F"], 0)
        f0_own += inv_n * nd["Fb"]
        Dm = [_mpf(b.D[k][i]) for k in range(nD)]
        for a in range(nu):
            acc = _Acc()
            for k in range(nD):
                if b.state[k] != a:
                    continue
                g = nd["G"][k]
                if g.t:
                    acc.add(Dm[k] * inv_n * g.v, 0)
                    acc.t += g.t
                    acc.a += Dm[k] * inv_n * (g.a - abs(g.v))
                    acc.b += Dm[k] * inv_n * g.b
                acc.add(Dm[k] * wi * _mpf(b.c[i, k]), 0)
            f1[a * n + i], f1b[a * n + i] = _f(acc.v), _f(acc.bound())
            for a2 in range(nu):
                acc = _Acc()
                for k in range(nD):
                    if b.state[k] != a:
                        continue
                    for k2 in range(nD):
                        h = nd["H"][k][k2]
                        if b.state[k2] != a2 or not h.t:
                            continue
                        acc.add(Dm[k] * inv_n * h.v * Dm[k2], 0)
                        acc.t += h.t
                        acc.a += Dm[k] * inv_n * (h.a - abs(h.v)) * Dm[k2]
                        acc.b += Dm[k] * inv_n * h.b * Dm[k2]
                f2[a * n + i, a2 * n + i], f2b[a * n + i, a2 * n + i] = _f(acc.v), _f(acc.bound())
    f0v = _f(f0.v) if inside.all() else np.inf
    f0b = _f(f0_own + (f0.t + 3) * U53 * f0.a)
    has_slack = not case.phase1
    return PointRef(Dz, inside, F, Fb, slack if has_slack else None, slackb if has_slack else None, f0v, f0b, f1, f1b, f2, f2b,
                    b.knode[pt])


# ---------------------------------------------------------------------------------------------------------------------
# fp64 evaluations held against the reference: the oracle, and the closed formulas with one deliberate error
# ---------------------------------------------------------------------------------------------------------------------

MUTATIONS = ("coef_qs_inv_r", "four_as_two", "pow_am2", "coef_qs_sign", "slack_to_q", "alpha_float", "drop_mu", "sign_aam1",
             "no_transpose", "gram_identity", "box_b_for_R", "lin_inv")
NEAR_WALL = ("coef_qs_inv_r", "four_as_two", "pow_am2", "coef_qs_sign", "slack_to_q", "no_transpose")        # the ones marked + in the issue
NEAR_K = 16


def applies(case, mut):
    b = built(case.name)
    eps = [pc for pc in b.Q.pieces if pc.kind == EP]
    wide = any(pc.ni > E.NARROW_W for pc in eps)
    if mut in ("slack_to_q", "box_b_for_R"):
        return case.phase1
    if mut == "alpha_float":
        return any(np.any(np.float32(2.0 / pc.p) != 2.0 / pc.p) for pc in eps)
    if mut == "sign_aam1":
        return any(np.any(pc.p != 2.0) for pc in eps)
    if mut == "no_transpose":
        return wide and any("A" in opt for _, _, opt in case.pieces)
    if mut == "gram_identity":
        return wide and any("A" in opt for _, _, opt in case.pieces)
    if mut == "lin_inv":
        return any(pc.kind == LIN for pc in b.Q.pieces)
    return True


def _ep_core_mut(mut):
    """oracle._ep_core with one deliberate error."""
    from oracle import mgb_oracle as O

    def core(q, s, p0, mu, order):
        with np.errstate(all="ignore"):
            alpha = 2.0 / p0
            if mut == "alpha_float":
                alpha = np.float32(alpha).astype(np.float64)
            qsq = np.sum(q * q, axis=1)
            r = O._safe_pow(s, alpha) - qsq
            if order == 0:
                return -O.Log(r) - mu * O.Log(s)
            inv_r = 1.0 / r
            s_am1 = O._safe_pow(s, alpha - 1.0)
            if order == 1:
                return np.concatenate([(2.0 * inv_r)[:, None] * q, (-alpha * s_am1 * inv_r - mu / s)[:, None]], axis=1)
            inv_r2 = inv_r * inv_r
            coef_qs = -2.0 * alpha * s_am1 * (inv_r if mut == "coef_qs_inv_r" else inv_r2)
            if mut == "coef_qs_sign":
                coef_qs = -coef_qs
            s_am2 = O._safe_pow(s, alpha - 2.0)
            s_2am2 = s_am2 if mut == "pow_am2" else O._safe_pow(s, 2.0 * alpha - 2.0)
            sg = 1.0 if mut == "sign_aam1" else -1.0
            H_ss = sg * alpha * (alpha - 1.0) * s_am2 * inv_r + alpha * alpha * s_2am2 * inv_r2 + (0.0 if mut == "drop_mu" else mu / (s * s))
            n, nq = q.shape
            H = np.zeros((n, nq + 1, nq + 1))
            H[:, :nq, :nq] = (2.0 if mut == "four_as_two" else 4.0) * q[:, :, None] * q[:, None, :] * inv_r2[:, None, None]
            for i in range(nq):
                H[:, i, i] += 2.0 * inv_r
            H[:, :nq, nq] = coef_qs[:, None] * q
            H[:, nq, :nq] = coef_qs[:, None] * q
            H[:, nq, nq] = H_ss
            return H
    return core


def wide_piece_hessian(pc, y, slack, mut=None):
    """A' H_z A of one EP piece by the algebra of wide_piece (csrc/cone.hpp), fp64: (2/r) A_q'A_q + (4/r^2) v v' +
    c_qs (v a_s' + a_s v') + H_ss a_s a_s', the upper triangle in the order of idx mirrored."""
    from oracle import mgb_oracle as O
    n, ni = y.shape[0], pc.ni
    A, q, s = O._ep_parts(pc, y, slack)
    Hz = O._ep_core(q, s, pc.p, pc.mu, 2)
    with np.errstate(all="ignore"):
        r = O._safe_pow(s, 2.0 / pc.p) - np.sum(q * q, axis=1)
        inv_r, inv_r2 = 1.0 / r, 1.0 / (r * r)
        cqs = -2.0 * (2.0 / pc.p) * O._safe_pow(s, 2.0 / pc.p - 1.0) * inv_r2
        Hss = Hz[:, ni - 1, ni - 1]
        Aq, a_s = A[:, :ni - 1, :], A[:, ni - 1, :]
        v = np.einsum("nrc,nr->nc", Aq, q)
        gram = np.einsum("nrc,nrd->ncd", Aq, Aq)
        if mut == "gram_identity":
            gram = np.broadcast_to(np.diag([1.0] * (ni - 1) + [0.0]), gram.shape)
        cross = v[:, :, None] * a_s[:, None, :]
        if mut != "no_transpose":
            cross = cross + a_s[:, :, None] * v[:, None, :]
        H = (2.0 * inv_r)[:, None, None] * gram + (4.0 * inv_r2)[:, None, None] * v[:, :, None] * v[:, None, :] + \
            cqs[:, None, None] * cross + Hss[:, None, None] * a_s[:, :, None] * a_s[:, None, :]
    order = np.argsort(np.argsort(pc.idx))
    up = order[:, None] <= order[None, :]
    return np.where(up[None], H, H.transpose(0, 2, 1))


def fp64_node_eval(name, pt, mut=None):
    """(F, G, H, slack) per node in fp64 at a point: the oracle's node_eval (mut None), or the same formulas with one error."""
    from oracle import mgb_oracle as O
    b = built(name)
    case = b.case
    Dz = dz_at(b, pt)
    NC = case.NC
    saved = (O._ep_core, O._ep_parts)
    try:
        if mut is not None:
            O._ep_core = _ep_core_mut(mut)
        if mut == "slack_to_q":
            orig = saved[1]

            def parts(pc, y, slack=None):
                A, q, s = orig(pc, y, None)
                return (A, q, s) if slack is None else (A, q + slack[:, None], s)
            O._ep_parts = parts
        with np.errstate(all="ignore"):
            F, G, H = (O.node_eval(b.Qo, Dz, k) for k in (0, 1, 2))
            if mut in ("no_transpose", "gram_identity", "wide_algebra"):
                yc = Dz[:, :NC] if case.phase1 else Dz
                for k, pc in enumerate(b.Q.pieces):
                    if pc.kind != EP:
                        continue
                    co = case.phase1
                    old = O._piece_eval(pc, yc, 2, co)
                    new = old.copy()
                    new[np.ix_(range(case.n), list(pc.idx), list(pc.idx))] = wide_piece_hessian(
                        pc, yc, yc[:, NC - 1] if co else None, None if mut == "wide_algebra" else mut)
                    act = np.ones(case.n, dtype=bool) if b.Q.select is None else b.Q.select[:, k] != 0
                    H[:, :yc.shape[1], :yc.shape[1]] += np.where(act[:, None, None], new - old, 0.0)
            if mut == "box_b_for_R":
                bb = b.box[0]
                v = Dz[:, NC:]
                G[:, NC:] = 1.0 / (bb - v) - 1.0 / (bb + v)
                for k in range(NC, case.nD):
                    H[:, k, k] = 1.0 / (bb - Dz[:, k]) ** 2 + 1.0 / (bb + Dz[:, k]) ** 2
            if mut == "lin_inv":
                yc = Dz[:, :NC] if case.phase1 else Dz
                for k, pc in enumerate(b.Q.pieces):
                    if pc.kind != LIN:
                        continue
                    nc, ni = pc.nc, pc.ni
                    A = pc.A.reshape(case.n, ni, nc).transpose(0, 2, 1)
                    Fv = np.einsum("nrc,nc->nr", A, yc[:, list(pc.idx)]) + pc.b
                    delta = 1.0 / Fv[:, 0] - 1.0 / Fv[:, 0] ** 2              # row 0: 1/Fv for 1/Fv^2
                    act = np.ones(case.n, dtype=bool) if b.Q.select is None else b.Q.select[:, k] != 0
                    H[np.ix_(range(case.n), list(pc.idx), list(pc.idx))] += np.where(
                        act[:, None, None], delta[:, None, None] * A[:, 0, :, None] * A[:, 0, None, :], 0.0)
            slack = None if case.phase1 else O.convex_slack(b.Q, Dz)
    finally:
        O._ep_core, O._ep_parts = saved
    return F, G, H, slack


def assemble_fp64(name, pt, F, G, H):
    """f0, f1 (nu n), f2 (nu n x nu n) from per-node F, G, H in fp64, the way Barrier.f0 / f1 / f2 form them (bw = 1/n)."""
    b = built(name)
    case = b.case
    n, nu, nD = case.n, case.nu, case.nD
    Dz = dz_at(b, pt)
    with np.errstate(all="ignore"):
        f0 = float(np.sum(F * (1.0 / n)) + np.sum(b.w * np.sum(b.c * Dz, axis=1)))
        Y = G * (1.0 / n) + b.w[:, None] * b.c
        f1 = np.zeros(nu * n)
        f2 = np.zeros((nu * n, nu * n))
        ar = np.arange(n)
        for k in range(nD):
            a = b.state[k]
            f1[a * n:(a + 1) * n] += b.D[k] * Y[:, k]
            for k2 in range(nD):
                a2 = b.state[k2]
                f2[a * n + ar, a2 * n + ar] += b.D[k] * (H[:, k, k2] * (1.0 / n)) * b.D[k2]
    return f0, f1, f2


def ratios(ref, F=None, slack=None, f0=None, f1=None, f2=None):
    """error / bound of whatever is given, at every entry of the nodes inside the cone: dict name -> (worst ratio, worst ratio
    over the entries of nodes with k >= NEAR_K).  A non-finite value where the reference is finite counts as +inf."""
    n = ref.inside.size
    nu = ref.f1.size // n
    ins = ref.inside
    near = ins & (ref.knode >= NEAR_K)
    out = {}

    def rr(d, v, bnd, mask):
        with np.errstate(all="ignore"):
            q = np.abs(d - v) / bnd
        q = np.where(np.isfinite(d), q, np.inf)
        q = np.where((bnd == 0) & (d == v), 0.0, q)
        return float(q[mask].max()) if mask.any() else 0.0

    if F is not None:
        out["F"] = (rr(F, ref.F, ref.Fb, ins), rr(F, ref.F, ref.Fb, near))
    if slack is not None and ref.slack is not None:
        out["slack"] = (rr(slack, ref.slack, ref.slackb, np.ones(n, dtype=bool)), rr(slack, ref.slack, ref.slackb, ref.knode >= NEAR_K))
    if f0 is not None and np.isfinite(ref.f0):
        out["f0"] = (abs(f0 - ref.f0) / ref.f0b if np.isfinite(f0) else np.inf, 0.0)
    if f1 is not None:
        m1, m2 = np.tile(ins, nu), np.tile(near, nu)
        out["f1"] = (rr(np.asarray(f1), ref.f1, ref.f1b, m1), rr(np.asarray(f1), ref.f1, ref.f1b, m2))
    if f2 is not None:
        f2 = np.asarray(f2)
        live = ref.f2b > 0
        assert np.all(f2[~live & np.tile(ins, nu)[:, None] & np.tile(ins, nu)[None, :]] == 0.0), "an entry with no term must be exactly zero"
        m1 = live & np.tile(ins, nu)[:, None]
        m2 = live & np.tile(near, nu)[:, None]
        out["f2"] = (rr(f2, ref.f2, ref.f2b, m1), rr(f2, ref.f2, ref.f2b, m2))
    return out
