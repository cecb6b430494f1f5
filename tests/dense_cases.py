"""Hand-built one-element problems that put every kernel of the dense-operator path (csrc/dense.hip; DESIGN.md "Shape gates")
on its tile, block and gate edges, with references whose componentwise bounds come from error analysis.

Layout.  N = 1 element of p = n nodes, `BlockDiag` operators of shape (n, n, 1), written out as plain dataclasses like
gate_cases.fem1d_problem.  "id" is the exact identity (`is_identity()` holds: the memcpy / hipMemcpy2DAsync branches); "dx"
(and "dy" of the wide case) are synthetic dense matrices, not Chebyshev ones: entry (i, k) = a(i) b(k) |weight| with
|weight| in [0.3, 0.95] rounded to 10 fractional bits and a, b mixed sign patterns.  u0 and every column of U carry the sign
b(k) of their node, so no row of dx (u0 + U s) and no entry of dx U cancels: every operator entry, every entry of D R and every
cone derivative is bounded away from zero, which is what lets the reference alone meet the sensitivity condition below.
The cone is the KIND_EP piece of gate_cases (p = 1.5) on D = [(0, "id"), (0, "dx"), (1, "id")]; the slack of z0 is an integer
>= 4 |dx u|^p at every node and level (well inside the cone: this file is about the linear algebra around the cone, not the
cone wall).  Coarse levels are R = blockdiag(U, S) with dense rounded U, S; the last level is the identity.

All of D, R, z0 and s are multiples of 2^-10, so z0 + R s, D (z0 + R s) and D R are exact in fp64 in any summation order.

References (u = 2^-53; the cone's per-node gradient Y_k and Hessian block Ybar come from the oracle in fp64 -- the project's
convention, KERNEL_RTOL its bar for them -- the linear algebra around them is formed in the 80-bit np.longdouble, or exactly
in rationals where the platform has no such type, and the reference's own rounding, the same gamma with 2^-64, is added):
  Dz = D_k (z0 + R s)            exact integers;       bound (n + len_row + 2) u (|D_k| (|z0| + |R| |s|))_i
  f1: g = R' sum_k D_k' Y_k                            bound ((n + len_j + nD + 2) u + KERNEL_RTOL) (|R|' sum_k |D_k|' |Y_k|)_j
  f2: H = (DR)' Ybar (DR)                              bound ((2 n + r n + r + 4) u + KERNEL_RTOL) A_ij,
      r active D rows, A = (|D||R|)' B (|D||R|), B the node blocks with every entry replaced by the block's largest modulus
      (the three gamma terms: plan GEMM, weight kernel, H GEMM; they hold for any summation order)
  f0: math.fsum of the oracle's per-node terms;        |f0_d - f0| <= KERNEL_RTOL |f0|, with sum |term| <= 4 |sum term|
An entry is checked only if its smallest non-zero term is >= SENSITIVITY x its bound; at most MAX_SKIPPED of a case's entries
may miss that, and none in the rows and columns NEVER_SKIPPED."""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

from gate_cases import KERNEL_RTOL, MAX_SKIPPED, P_CONE, SENSITIVITY, U53, weight

EXTENDED = np.finfo(np.longdouble).nmant == 63        # the x87 80-bit type; elsewhere the sums are formed exactly (Fraction)
UREF = 2.0 ** -64 if EXTENDED else 0.0                # unit roundoff of the reference's own sums
BITS = 10
ONE = 1 << BITS
GT, GK = 64, 16                                       # csrc/dense.hip: tile edge and K tile of dense_gemm_tn_kernel
NEVER_SKIPPED = (0, 62, 63, 64, 65, 127, 128, -1)     # rows / columns on the 64-tile edges; -1: the last one, m - 1
MASKED_NODES = (0, 63, 64, 255, 256)


def rnd(v):
    return np.round(np.asarray(v, dtype=np.float64) * ONE) / ONE


def sign(i, salt):
    """A fixed mixed +-1 pattern."""
    return np.where(np.sin(1.7 * np.asarray(i, dtype=np.float64) + salt) < 0.0, -1.0, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Case:
    name: str
    n: int
    coarse: list                       # columns per state and coarse level: [(cu, cs)] or [(cu1, cu2, cs)]
    claims: dict                       # what the case is for, asserted by check_claims
    kind: str = "plain"                # "plain" | "wide" | "masked" | "dx_first"

    @property
    def nu(self):
        return 3 if self.kind == "wide" else 2

    @property
    def D_spec(self):
        if self.kind == "wide":        # Zoo.p_harmonic in 2-D: per component an id row and two partials, then the slack
            return [(0, "id"), (0, "dx"), (0, "dy"), (1, "id"), (1, "dx"), (1, "dy"), (2, "id")]
        if self.kind == "dx_first":
            return [(0, "dx"), (0, "id"), (1, "id")]
        return [(0, "id"), (0, "dx"), (1, "id")]

    @property
    def idx(self):
        return (1, 2, 4, 5, 6) if self.kind == "wide" else (0, 2) if self.kind == "dx_first" else (1, 2)

    @property
    def active(self):
        """(klo, khi): the contiguous range of D rows that enter the barrier (problem.cpp: eval_f2)."""
        return min(self.idx), max(self.idx)

    @property
    def sizes(self):
        return [sum(c) for c in self.coarse] + [self.nu * self.n]


def _split(m):
    return (m // 2, m - m // 2)


CASES = [
    # the element-kernel side of the `p > 64` gate (kernels.hip), same problem formulas and the same bounds
    Case("n64", 64, [_split(63), _split(64), _split(65)], dict(dense=False, tiles={63: 1, 64: 1, 65: 2}, edge={65: 1})),
    # smallest dense n: empty waves 13-15 in gemv_n (cw = 5), one row past a 64-row block, K tails 65 % 16 and 130 % 16,
    # nkt = 5 and 9, GEMM M = 63 / 64 / 65 (1 tile, exact tile, 2 x 2 tiles with a width-1 edge and its mirror)
    Case("n65", 65, [(1, 1), _split(63), _split(64), _split(65)],
         dict(dense=True, gemv_cw=5, gemv_empty_waves=(13, 14, 15), row_blocks=2, last_row_block=1, ktail_plan=1, ktail_H=2,
              nkt_plan=5, nkt_H=9, tiles={2: 1, 63: 1, 64: 1, 65: 2}, edge={63: 63, 64: 64, 65: 1})),
    # H product K = 2 * 96 = 192: nkt = 12, nkt % 3 == 0; plan product nkt = 6, also 0 mod 3
    Case("n96", 96, [_split(65)], dict(dense=True, nkt_plan=6, nkt_H=12, nkt_plan_mod3=0, nkt_H_mod3=0, ktail_plan=0, ktail_H=0,
                                       tiles={65: 2}, edge={65: 1})),
    # 64-row blocks 2 + 1; M = 128 (2 x 2 exact tiles), 129 (3 x 3 with a width-1 edge)
    Case("n129", 129, [_split(128), _split(129)], dict(dense=True, row_blocks=3, last_row_block=1, tiles={128: 2, 129: 3},
                                                       edge={128: 64, 129: 1})),
    # exactly one full node block
    Case("n256", 256, [_split(65)], dict(dense=True, node_blocks=1, last_node_block=256, tiles={65: 2}, edge={65: 1})),
    # second node block with one active thread, two f0 partials, gemv_t rows = 4 * 64 + 1
    Case("n257", 257, [_split(65), _split(129)], dict(dense=True, node_blocks=2, last_node_block=1, gemv_t_tail=1, row_blocks=5,
                                                      last_row_block=1, tiles={65: 2, 129: 3}, edge={65: 1, 129: 1})),
    # dense_node_wide_kernel: a vector problem shaped like Zoo.p_harmonic in 2-D (nu = 3, seven D rows, one EP piece of
    # width 5 > NARROW_W) on the synthetic id / dx / dy
    Case("n257_wide", 257, [(22, 22, 21)], dict(dense=True, wide=True, node_blocks=2, last_node_block=1, active_rows=6,
                                                tiles={65: 2}, edge={65: 1}), kind="wide"),
    # barrier weights bw: 0 at nodes {0, 63, 64, 255, 256}, rounded non-unit values elsewhere
    Case("n257_masked", 257, [_split(65)], dict(dense=True, node_blocks=2, last_node_block=1, tiles={65: 2}, edge={65: 1}),
         kind="masked"),
    # D rows in the order (dx, id, id): the first row of state u is not the identity, so its restriction starts with
    # dense_gemv_t_kernel<false> (every other case copies the identity row and then adds); the inactive id row lies inside
    # the active range 0 .. 2, so the H product runs over K = 3 * 65 = 195 (nkt = 13) with a block of zero weights
    Case("n65_dx_first", 65, [_split(65)], dict(dense=True, active_rows=3, nkt_H=13, ktail_H=3, tiles={65: 2}, edge={65: 1}),
         kind="dx_first"),
]
CASE = {c.name: c for c in CASES}
LEVELS = [(c.name, l) for c in CASES for l in range(len(c.sizes))]


def shape_facts(case, m):
    """The tile, block and ring arithmetic of csrc/dense.hip for one level, from n, m and the active-row range."""
    n = case.n
    klo, khi = case.active
    r = khi - klo + 1
    cw = -(-n // 16)
    T = -(-m // GT)
    return dict(gemv_cw=cw, gemv_empty_waves=tuple(w for w in range(16) if w * cw >= n), row_blocks=-(-n // 64),
                last_row_block=n - 64 * (-(-n // 64) - 1), node_blocks=-(-n // 256), last_node_block=n - 256 * (-(-n // 256) - 1),
                gemv_t_tail=n % 64, nkt_plan=-(-n // GK), nkt_H=-(-(r * n) // GK), ktail_plan=n % GK, ktail_H=(r * n) % GK,
                active_rows=r, tiles=T, edge=m - GT * (T - 1))


def check_claims(case):
    """Every literal of `claims` against the arithmetic: a later edit cannot let a case slip off its edge."""
    cl = case.claims
    assert cl["dense"] == (case.n > 64), case.name
    assert cl.get("wide", False) == (len(case.idx) > 4), case.name
    facts = {m: shape_facts(case, m) for m in case.sizes}
    first = facts[case.sizes[0]]
    for key, want in cl.items():
        if key in ("dense", "wide"):
            continue
        if key in ("tiles", "edge"):
            for m, v in want.items():
                assert m in case.sizes[:-1] and facts[m][key] == v, (case.name, key, m, facts[m][key], v)
        elif key.endswith("_mod3"):
            assert first[key[:-5]] % 3 == want, (case.name, key)
        else:
            assert first[key] == want, (case.name, key, first[key], want)
    return True


for _c in CASES:
    check_claims(_c)


# ---------------------------------------------------------------------------------------------------------------------
# the problems
# ---------------------------------------------------------------------------------------------------------------------

_A_SALT = {"dx": 0.4, "dy": 2.9}
_W_SALT = {"dx": (17, 1), "dy": (23, 4)}


def operator(name, n):
    i, k = np.arange(n)[:, None], np.arange(n)[None, :]
    if name == "id":
        return np.eye(n)
    f, j0 = _W_SALT[name]
    return sign(i, _A_SALT[name]) * sign(k, 1.3) * rnd(weight(f * i + 3 * k, j0 + 0 * k))


def _U(n, cols, salt):
    k, i = np.arange(n)[:, None], np.arange(cols)[None, :]
    return sign(k, 1.3) * sign(i, salt) * rnd(weight(11 * k + 5, 3 * i + salt)), sign(np.arange(cols), salt)


def _S(n, cols):
    k, j = np.arange(n)[:, None], np.arange(cols)[None, :]
    return sign(k, 0.7) * sign(j, 2.2) * rnd(weight(7 * k + 2, 5 * j + 3)), sign(np.arange(cols), 2.2)


@dataclass
class Built:
    case: Case
    ops: dict
    D: list                            # nD dense (n x n) operators
    state: list                        # state of every D row
    R: list                            # per level: dense (nu n x m)
    cols: list                         # per level: [(start, stop)] column range of every state
    s: list                            # per level: the coarse vector
    z0: np.ndarray
    w: np.ndarray
    c: np.ndarray
    bw: object
    M: object = field(repr=False, default=None)
    Q: object = field(repr=False, default=None)


@functools.lru_cache(maxsize=None)
def built(name):
    from mgb_amd.blockmatrices import BlockColumn, BlockDiag
    from mgb_amd.convex import KIND_EP, Convex, Piece
    from mgb_amd.multigrid import AMG, Geometry
    case = CASE[name]
    n, nu = case.n, case.nu
    nodes = np.arange(n)
    names = sorted({nm for _, nm in case.D_spec})
    ops = {nm: operator(nm, n) for nm in names}
    D = [ops[nm] for _, nm in case.D_spec]
    state = [a for a, _ in case.D_spec]
    nD = len(D)
    # levels: blockdiag of dense rounded blocks, then the identity; s: 1 .. 3 units of 2^-10 with the sign of its column
    R, cols, svec = [], [], []
    for widths in case.coarse:
        blocks, signs = [], []
        for a, cw in enumerate(widths):
            B, sg = _S(n, cw) if a == nu - 1 else _U(n, cw, 0.9 + 2.0 * a)
            blocks.append(B); signs.append(sg)
        R.append(np.asarray(sp.block_diag(blocks).todense()))
        edges = np.concatenate([[0], np.cumsum(widths)])
        cols.append([(int(edges[a]), int(edges[a + 1])) for a in range(nu)])
        sg = np.concatenate(signs)
        svec.append(sg * (1 + np.arange(sg.size) % 3) / ONE)
    R.append(np.eye(nu * n))
    cols.append([(a * n, (a + 1) * n) for a in range(nu)])
    sg = np.concatenate([sign(nodes, 1.3)] * (nu - 1) + [sign(nodes, 0.7)])
    svec.append(sg * (1 + np.arange(sg.size) % 3) / ONE)
    # z0 = (u, s): u with the sign of its node; s an integer >= 4 |q|^p at every node and level
    us = [sign(nodes, 1.3) * rnd(weight(3 * nodes + 40 * a, 1 + a) / 8) for a in range(nu - 1)]
    qmax = 0.0
    for Rl, sl in zip(R, svec):
        zl = np.concatenate(us + [np.zeros(n)]) + Rl @ sl
        q2 = sum((D[k] @ zl[state[k] * n:(state[k] + 1) * n]) ** 2 for k in case.idx[:-1])
        qmax = max(qmax, float(np.sqrt(q2.max())))
    base = 2 ** math.ceil(math.log2(4.0 * qmax ** P_CONE))
    z0 = np.concatenate(us + [base + 4.0 * (nodes % 5)])
    w = np.round(weight(nodes, 2) * ONE) / (ONE * 256)
    c = np.stack([sign(nodes, 0.3 + k) * rnd(weight(2 * nodes + k, k + 4)) for k in range(nD)], axis=1)
    c[:, nD - 1] = -np.abs(c[:, nD - 1])          # the slack row: the linear part has the sign of the barrier (f0 does not cancel)
    bw = None
    if case.kind == "masked":
        bw = np.round(weight(5 * nodes, 2) * 64) / 16384
        bw[list(MASKED_NODES)] = 0.0
    blk = {nm: BlockDiag(ops[nm].reshape(n, n, 1)) for nm in names}
    dim = 2 if case.kind == "wide" else 1
    x = np.stack([np.cos(math.pi * (nodes + 0.5) / n), np.sin(0.9 * nodes)], axis=1)[:, :dim]
    geom = Geometry(discretization=None, t=nodes.reshape(n, 1), x=x.reshape(n, 1, dim).copy(), w=w, operators=blk)
    M = AMG(geometry=geom, x=x.copy(), w=w, R_fine=[sp.csr_matrix(Rl) for Rl in R],
            D_fine=[BlockColumn(blk[nm], a, nu) for a, nm in case.D_spec],
            state_names=["u1", "u2", "s"] if nu == 3 else ["u", "s"], D_spec=list(case.D_spec))
    ni = len(case.idx)
    Q = Convex([Piece(KIND_EP, case.idx, np.tile(np.eye(ni).reshape(-1), (n, 1)), np.zeros((n, ni)), np.full(n, P_CONE),
                      np.full(n, 1.0))])
    return Built(case, ops, D, state, R, cols, svec, z0, w, c, bw, M, Q)


def inputs(name, level):
    b = built(name)
    return b.s[level], b.c, b.z0


# ---------------------------------------------------------------------------------------------------------------------
# checked entries
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Reference:
    """One operation on one level: value, componentwise bound, sum of |terms| and the smallest non-zero |term| per entry,
    all in the shape of the device's output; never: entries that may not miss the sensitivity condition."""
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
        return 1.0 - float(self.sensitive[live].mean())

    def ratios(self, device_values):
        """|device - reference| / bound on the entries that meet the sensitivity condition (entries with no term: exact 0)."""
        d = np.asarray(device_values, dtype=np.float64).reshape(self.value.shape)
        empty = self.abssum == 0
        assert np.all(d[empty] == 0.0), "an entry with no term must be exactly zero"
        use = self.sensitive & ~empty
        return np.abs(d[use] - self.value[use]) / self.bound[use]


def never_mask(shape, axes):
    """True on the NEVER_SKIPPED indices of every axis in `axes`."""
    mask = np.zeros(shape, dtype=bool)
    for ax in axes:
        size = shape[ax]
        pick = sorted({i % size for i in NEVER_SKIPPED if -size <= i < size})
        sl = [slice(None)] * len(shape)
        sl[ax] = pick
        mask[tuple(sl)] = True
    return mask


def _ints(a):
    """Multiples of 2^-10 as int64, exactly."""
    v = np.asarray(a, dtype=np.float64) * ONE
    q = np.rint(v).astype(np.int64)
    assert np.array_equal(q.astype(np.float64), v)
    return q


def _x(a):
    """Into the reference's working type."""
    a = np.asarray(a, dtype=np.float64)
    if EXTENDED:
        return a.astype(np.longdouble)
    return np.frompyfunc(Fraction, 1, 1)(a).astype(object)


def _f(a):
    return np.asarray(a, dtype=np.float64) if EXTENDED else np.frompyfunc(float, 1, 1)(a).astype(np.float64)


def _minprod(X, Z):
    """min over nodes of X[node, i] Z[node, j] over the non-zero products (inf where there is none); X, Z >= 0."""
    out = np.full((X.shape[1], Z.shape[1]), np.inf)
    for xr, zr in zip(X, Z):
        t = xr[:, None] * zr[None, :]
        np.minimum(out, np.where(t > 0, t, np.inf), out=out)
    return out


@functools.lru_cache(maxsize=None)
def dz_reference(name, level):
    """(z, Reference): z = z0 + R s exactly (the identity rows of Dz are these bits), Dz[:, k] = D_k z_state(k) exactly."""
    b = built(name)
    n, nD = b.case.n, len(b.D)
    Ri, si, z0i = _ints(b.R[level]), _ints(b.s[level]), _ints(b.z0)
    zi = z0i * ONE + Ri @ si                                         # units of 2^-20
    za = np.abs(z0i) * ONE + np.abs(Ri) @ np.abs(si)
    val, ab, mn, ln = (np.zeros((n, nD)) for _ in range(4))
    for k, Dk in enumerate(b.D):
        a = b.state[k]
        Di = _ints(Dk)
        val[:, k] = (Di @ zi[a * n:(a + 1) * n]).astype(np.float64) / float(ONE ** 3)      # |.| < 2^53: exact
        terms = np.abs(Di) * za[None, a * n:(a + 1) * n]
        ab[:, k] = terms.sum(axis=1).astype(np.float64) / float(ONE ** 3)
        mn[:, k] = np.where(terms > 0, terms, np.iinfo(np.int64).max).min(axis=1).astype(np.float64) / float(ONE ** 3)
        ln[:, k] = np.count_nonzero(Di, axis=1)
    z = zi.astype(np.float64) / float(ONE * ONE)
    return z, Reference(val, (n + ln + 2) * U53 * ab, ab, mn, never_mask((n, nD), (0,)))


@functools.lru_cache(maxsize=None)
def oracle_node(name, level):
    """The oracle's fp64 per-node quantities at the exact Dz: F (n), Y (n x nD: scaled gradient + w c), Ybar (n x nD x nD),
    the slack, and the per-node terms of f0."""
    from oracle import mgb_oracle as O
    b = built(name)
    Dz = dz_reference(name, level)[1].value
    B = O.Barrier(b.Q, b.bw)
    n = b.case.n
    F = O.node_eval(b.Q, Dz, 0)
    Y = B._scale(n, O.node_eval(b.Q, Dz, 1)) + b.w[:, None] * b.c
    Ybar = B._scale(n, O.node_eval(b.Q, Dz, 2))
    terms = B._scale(n, F) + b.w * np.sum(b.c * Dz, axis=1)
    return dict(Dz=Dz, F=F, Y=Y, Ybar=Ybar, slack=O.convex_slack(b.Q, Dz), f0_terms=terms)


def f0_reference(name, level):
    """(f0, sum |term|): math.fsum of the oracle's per-node terms."""
    t = oracle_node(name, level)["f0_terms"]
    return math.fsum(t.tolist()), math.fsum(np.abs(t).tolist())


@functools.lru_cache(maxsize=None)
def f1_reference(name, level):
    b = built(name)
    n, nD, nu = b.case.n, len(b.D), b.case.nu
    Y = oracle_node(name, level)["Y"]
    R = b.R[level]
    m = R.shape[1]
    val, ab, mn = np.zeros(m), np.zeros(m), np.full(m, np.inf)
    for a in range(nu):
        j0, j1 = b.cols[level][a]
        Ra = R[a * n:(a + 1) * n, j0:j1]
        ret, reta = _x(np.zeros(n)), np.zeros(n)
        for k in range(nD):
            if b.state[k] != a:
                continue
            ret = ret + _x(b.D[k].T) @ _x(Y[:, k])
            T = np.abs(b.D[k]) * np.abs(Y[:, k])[:, None]                      # |D_k[node, a'] Y_k[node]|
            reta += T.sum(axis=0)
            v = np.where(T > 0, T, np.inf).min(axis=0)                         # per fine row a': its smallest non-zero term
            pr = np.abs(Ra) * v[:, None]
            mn[j0:j1] = np.minimum(mn[j0:j1], np.where(pr > 0, pr, np.inf).min(axis=0))
        val[j0:j1] = _f(_x(Ra.T) @ ret)
        ab[j0:j1] = np.abs(Ra).T @ reta
    ln = np.count_nonzero(R, axis=0)
    bound = ((n + ln + nD + 2) * (U53 + UREF) + KERNEL_RTOL) * ab * (1.0 + 2.0 ** -40)
    return Reference(val, bound, ab, mn, never_mask((m,), (0,)))


def DR_exact(name, level):
    """DR_k = D_k R[rows of state(k)] restricted to the columns of that state (the others are structurally zero), exact."""
    b = built(name)
    n = b.case.n
    out = []
    for k, Dk in enumerate(b.D):
        a = b.state[k]
        j0, j1 = b.cols[level][a]
        P = _ints(Dk) @ _ints(b.R[level][a * n:(a + 1) * n, j0:j1])
        out.append(P.astype(np.float64) / float(ONE * ONE))
    return out


@functools.lru_cache(maxsize=None)
def f2_reference(name, level):
    b = built(name)
    n, case = b.case.n, b.case
    klo, khi = case.active
    r = khi - klo + 1
    Ybar = oracle_node(name, level)["Ybar"]
    DR = DR_exact(name, level)
    m = b.R[level].shape[1]
    Bmax = np.abs(Ybar).max(axis=(1, 2))
    val, A, mn = np.zeros((m, m)), np.zeros((m, m)), np.full((m, m), np.inf)
    xDR = {k: _x(DR[k]) for k in range(klo, khi + 1)}
    for k in range(klo, khi + 1):
        i0, i1 = b.cols[level][b.state[k]]
        for k2 in range(klo, khi + 1):
            j0, j1 = b.cols[level][b.state[k2]]
            A[i0:i1, j0:j1] += np.abs(DR[k]).T @ (Bmax[:, None] * np.abs(DR[k2]))
            y = Ybar[:, k, k2]
            if not np.any(y):
                continue
            val[i0:i1, j0:j1] += _f(xDR[k].T @ (_x(y)[:, None] * xDR[k2]))
            blk = mn[i0:i1, j0:j1]
            np.minimum(blk, _minprod(np.abs(DR[k]) * np.abs(y)[:, None], np.abs(DR[k2])), out=blk)
    # block sums in fp64: at most r^2 additions of rounded longdouble results -- covered by the 2^-40 slack of the bound
    live = np.isfinite(mn)
    ab = np.where(live, A, 0.0)
    bound = ((2 * n + r * n + r + 4) * (U53 + UREF) + KERNEL_RTOL) * A * (1.0 + 2.0 ** -40)
    return Reference(val, bound, ab, mn, never_mask((m, m), (0, 1)))


def f2_terms(name, level, i, j):
    """Every term of H_ij in the K order of the H GEMM (K index = (k - klo) n + node), as (K index, value) arrays; the value
    is DR_k[node, i] sum_k2 Ybar[node, k, k2] DR_k2[node, j] split over k2."""
    b = built(name)
    n = b.case.n
    klo, khi = b.case.active
    Ybar = oracle_node(name, level)["Ybar"]
    DR = DR_exact(name, level)

    def column(k, col):
        c0, c1 = b.cols[level][b.state[k]]
        return DR[k][:, col - c0] if c0 <= col < c1 else np.zeros(n)
    kidx, vals = [], []
    for k in range(klo, khi + 1):
        for k2 in range(klo, khi + 1):
            kidx.append((k - klo) * n + np.arange(n))
            vals.append(column(k, i) * Ybar[:, k, k2] * column(k2, j))
    return np.concatenate(kidx), np.concatenate(vals)


def oracle_closures(name, level):
    """O.Barrier's own f0 / f1 / f2 of the level."""
    from oracle import mgb_oracle as O
    b = built(name)
    Mo = O.OracleAMG(b.M)
    B = O.Barrier(b.Q, b.bw)
    s, c, z0 = inputs(name, level)
    args = (s, Mo.w, c, Mo.R_fine[level], Mo.D_fine, z0)
    return B.f0(*args), B.f1(*args), np.asarray(sp.csr_matrix(B.f2(*args)).todense())
