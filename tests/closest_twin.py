"""A plain NumPy restatement of `closest_point()` / `ClosestPointLocator` (csrc/closest.hip): the yardstick of
tests/test_closest.py and tests/test_gpu_closest.py.

For every point EVERY element is projected (no grid, no candidate lists), by the method of the device kernel:

1. start at the element's node nearest to the point (the first one on a tie, nodes in storage order);
2. minimise f(xi) = |x(xi) - q|^2 / 2 over [-1, 1]^d.  With r = x(xi) - q, J = dx/dxi, g = J^T r, A = J^T J and
   C[b][c] = r . d^2x / dxi_b dxi_c: a coordinate on a bound whose descent direction -g points out of the cube is frozen;
   on the free coordinates the step solves H s = -g with the full Hessian H = A + C where that is positive definite and
   with the Gauss-Newton matrix A otherwise; xi <- clamp(xi + s).  An iterate whose |r|^2 exceeds that of the last
   accepted one by more than the rounding level of |r|^2 is rejected: the step from the accepted iterate is halved
   instead (a rejection counts as an iteration, and a step halved below the tolerance of 3. ends the iteration there);
3. stop once max|step| <= max(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * max|x| * |(J^T J)^-1 J^T|_inf), after `maxit`
   iterations (200 here, 64 on the device), or when J^T J is singular or a step is not finite;
4. the candidate's distance is |x(xi) - q| at its last iterate, converged or not.

Every sum over an element's nodes runs over x_i - x_0, the nodes relative to the element's first one (sum phi_i = 1, sum
dphi_i = 0), and r = sum phi_i (x_i - x_0) - (q - x_0), foot = x_0 + sum phi_i (x_i - x_0): exact differences on a small
element far from the origin.

The winner is the smallest squared distance, the lowest element index on a tie; a winner farther than `max_distance`
leaves the point without an element.  Per point the twin reports `margin` (second-best minus best distance) and keeps the
result of every element, so that a comparison can look at the element the device chose where two elements tie.
"""
from dataclasses import dataclass

import numpy as np

from mgb_amd.tensorfem import _tf_nodes

EPS = 2.220446049250313e-16
ROUND_FACTOR = 64.0
NEWTON_STEP_TOL = 1e-13
BOX_PAD = 0.125                  # csrc/interp_device.hpp QK_BOX_PAD
TWIN_MAXIT = 200
DEVICE_MAXIT = 64


def lagrange_dd(nodes, xv):
    """(L, dL, ddL), each (B, S): the 1-D Lagrange basis on `nodes` and its first two derivatives at xv (B,)."""
    S = len(nodes)
    xv = np.asarray(xv, dtype=np.float64)
    L, dL, ddL = (np.empty(xv.shape + (S,)) for _ in range(3))
    for i in range(S):
        num, dnum, ddnum, den = np.ones_like(xv), np.zeros_like(xv), np.zeros_like(xv), 1.0
        for j in range(S):
            if i != j:
                t = xv - nodes[j]
                ddnum = ddnum * t + 2.0 * dnum
                dnum = dnum * t + num
                num = num * t
                den *= nodes[i] - nodes[j]
        L[..., i], dL[..., i], ddL[..., i] = num / den, dnum / den, ddnum / den
    return L, dL, ddL


def basis(nodes, xi):
    """phi (B, P), dphi (B, d, P), ddphi (B, d, d, P) of the tensor basis at xi (B, d); node lin = i0 + S i1."""
    B, d = xi.shape
    L0, d0, dd0 = lagrange_dd(nodes, xi[:, 0])
    if d == 1:
        return L0, d0[:, None, :], dd0[:, None, None, :]
    L1, d1, dd1 = lagrange_dd(nodes, xi[:, 1])

    def outer(a1, a0):
        return (a1[:, :, None] * a0[:, None, :]).reshape(B, -1)
    phi = outer(L1, L0)
    dphi = np.stack([outer(L1, d0), outer(d1, L0)], axis=1)
    m = outer(d1, d0)
    ddphi = np.stack([np.stack([outer(L1, dd0), m], axis=1), np.stack([m, outer(dd1, L0)], axis=1)], axis=1)
    return phi, dphi, ddphi


def _pinv_norm(J):
    """(|(J^T J)^-1 J^T|_inf, usable) of J (B, e, d)."""
    d = J.shape[2]
    A = np.einsum("bac,bad->bcd", J, J)
    with np.errstate(all="ignore"):
        if d == 1:
            det = A[:, 0, 0]
            ninv = np.abs(J[:, :, 0]).sum(axis=1) / det
        else:
            det = A[:, 0, 0] * A[:, 1, 1] - A[:, 0, 1] * A[:, 0, 1]
            P0 = (A[:, 1, 1, None] * J[:, :, 0] - A[:, 0, 1, None] * J[:, :, 1]) / det[:, None]
            P1 = (A[:, 0, 0, None] * J[:, :, 1] - A[:, 0, 1, None] * J[:, :, 0]) / det[:, None]
            ninv = np.maximum(np.abs(P0).sum(axis=1), np.abs(P1).sum(axis=1))
        ok = (det > 0) & np.isfinite(det) & np.isfinite(ninv)
    return ninv, ok, A


def project(Xe, q, nodes, maxit=TWIN_MAXIT):
    """Every row b: the point q[b] (e,) projected onto the element with nodes Xe[b] (P, e).
    Returns xi (B, d), foot (B, e), d2 (B,), conv (B,), its (B,)."""
    B, P, e = Xe.shape
    S = len(nodes)
    d = 1 if P == S else 2
    near = np.argmin(((Xe - q[:, None, :]) ** 2).sum(axis=2), axis=1)
    xi = np.stack([nodes[near % S]] + ([nodes[near // S]] if d == 2 else []), axis=1).astype(np.float64)
    xs = np.maximum(np.abs(Xe).reshape(B, -1).max(axis=1), np.abs(q).max(axis=1))
    X0 = Xe[:, 0, :]
    Xs, qs = Xe - X0[:, None, :], q - X0                               # relative to the element's first node
    rn = ROUND_FACTOR * EPS * xs                                      # rounding level of a component of r
    active, conv, its = np.ones(B, dtype=bool), np.zeros(B, dtype=bool), np.zeros(B, dtype=np.int64)
    xa, fa, sa, ta = xi.copy(), np.full(B, np.inf), np.zeros_like(xi), np.zeros(B)   # the last accepted iterate
    for _ in range(maxit):
        ix = np.nonzero(active)[0]
        if ix.size == 0:
            break
        its[ix] += 1
        x0 = xi[ix]
        phi, dphi, ddphi = basis(nodes, x0)
        X = Xs[ix]
        r = np.einsum("bp,bpa->ba", phi, X) - qs[ix]
        f = (r * r).sum(axis=1)
        with np.errstate(all="ignore"):
            rej = f > fa[ix] + 4.0 * rn[ix] * (np.sqrt(fa[ix]) + rn[ix])       # false while fa is inf
        if rej.any():                                                # the step went uphill: halve it from the accepted point
            jx = ix[rej]
            sa[jx] *= 0.5
            small = np.abs(sa[jx]).max(axis=1) <= ta[jx]
            xi[jx] = np.where(small[:, None], xa[jx], xa[jx] + sa[jx])
            conv[jx[small]] = True
            active[jx[small]] = False
            keep = ~rej
            ix, x0, dphi, ddphi, X, r, f = ix[keep], x0[keep], dphi[keep], ddphi[keep], X[keep], r[keep], f[keep]
            if ix.size == 0:
                continue
        J = np.einsum("bcp,bpa->bac", dphi, X)                       # (b, e, d)
        g = np.einsum("bac,ba->bc", J, r)
        Cm = np.einsum("bcdp,bpa,ba->bcd", ddphi, X, r)
        ninv, ok, A = _pinv_norm(J)
        fr = ((x0 <= -1.0) & (g > 0.0)) | ((x0 >= 1.0) & (g < 0.0))
        with np.errstate(all="ignore"):
            if d == 1:
                h = A[:, 0, 0] + Cm[:, 0, 0]
                h = np.where(h > 0.0, h, A[:, 0, 0])
                s = np.where(fr, 0.0, -g / h[:, None])
            else:
                H = A + Cm
                det = H[:, 0, 0] * H[:, 1, 1] - H[:, 0, 1] * H[:, 0, 1]
                full = (H[:, 0, 0] > 0.0) & (det > 0.0)
                H = np.where(full[:, None, None], H, A)
                det = H[:, 0, 0] * H[:, 1, 1] - H[:, 0, 1] * H[:, 0, 1]
                both = np.stack([-(H[:, 1, 1] * g[:, 0] - H[:, 0, 1] * g[:, 1]) / det,
                                 -(H[:, 0, 0] * g[:, 1] - H[:, 0, 1] * g[:, 0]) / det], axis=1)
                hd = np.stack([A[:, 0, 0] + Cm[:, 0, 0], A[:, 1, 1] + Cm[:, 1, 1]], axis=1)
                hd = np.where(hd > 0.0, hd, np.stack([A[:, 0, 0], A[:, 1, 1]], axis=1))
                one = -g / hd
                nfr = fr.sum(axis=1)
                s = np.where(fr, 0.0, np.where((nfr == 0)[:, None], both, one))
            ok = ok & np.isfinite(s).all(axis=1)
            xn = np.clip(x0 + s, -1.0, 1.0)
            s = xn - x0
            step = np.abs(s).max(axis=1)
            tol = np.maximum(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * xs[ix] * ninv)
            done = ok & (step <= tol)
        jx = ix[ok]
        xa[jx], fa[jx], sa[jx], ta[jx] = x0[ok], f[ok], s[ok], tol[ok]
        xi[jx] = xn[ok]
        conv[ix[done]] = True
        active[ix[done | ~ok]] = False
    phi, _, _ = basis(nodes, xi)
    rel = np.einsum("bp,bpa->ba", phi, Xs)
    foot = X0 + rel
    d2 = ((rel - qs) ** 2).sum(axis=1)
    return xi, foot, d2, conv, its


def default_max_distance(geom) -> float:
    """0.125 x the largest diagonal of an element's node box."""
    x = np.asarray(geom.x, dtype=np.float64)                         # (p, N, e)
    ext = x.max(axis=0) - x.min(axis=0)
    return float(BOX_PAD * np.sqrt((ext * ext).sum(axis=1)).max())


@dataclass
class TwinClosest:
    geom: object
    nodes: np.ndarray
    max_distance: float
    elements: np.ndarray      # (M,) int32, -1: none
    xi: np.ndarray            # (M, d), NaN where elements == -1
    points: np.ndarray        # (M, e)
    distances: np.ndarray     # (M,)
    converged: np.ndarray     # (M,) bool: the winner's iteration met its stopping test
    margin: np.ndarray        # (M,): second-best minus best distance over the elements (inf for one element)
    all_xi: np.ndarray        # (M, N, d): the result of every element
    all_points: np.ndarray    # (M, N, e)
    all_distances: np.ndarray  # (M, N)
    all_converged: np.ndarray  # (M, N)
    all_iterations: np.ndarray  # (M, N)

    def _at(self, elem, xi):
        """(phi, dphi, the element's nodes (M, P, e), the rows of z it owns) at (elem, xi); elem >= 0."""
        p, N, e = self.geom.x.shape
        phi, dphi, _ = basis(self.nodes, xi)
        X = np.asarray(self.geom.xflat, dtype=np.float64).reshape(N, p, e)[elem]
        rows = elem[:, None] * p + np.arange(p)[None, :]
        return phi, dphi, X, rows

    def evaluate(self, z, elements=None, xi=None, gradient=False):
        """Values (M, ncomp) and, with `gradient`, tangential gradients (M, ncomp, e) at the twin's feet, or at the given
        (elements, xi); NaN where the element is -1."""
        elem = self.elements if elements is None else np.asarray(elements)
        xi = self.xi if xi is None else np.asarray(xi, dtype=np.float64)
        Z = np.asarray(z, dtype=np.float64)
        Z = Z.reshape(Z.shape[0], -1)
        M, e = elem.shape[0], self.geom.x.shape[2]
        ok = elem >= 0
        vals = np.full((M, Z.shape[1]), np.nan)
        grads = np.full((M, Z.shape[1], e), np.nan)
        if ok.any():
            phi, dphi, X, rows = self._at(elem[ok], xi[ok])
            Ze = Z[rows]                                              # (m, P, ncomp)
            vals[ok] = np.einsum("bp,bpc->bc", phi, Ze)
            if gradient:
                J = np.einsum("bdp,bpa->bad", dphi, X - X[:, :1])     # (m, e, d)
                gxi = np.einsum("bdp,bpc->bcd", dphi, Ze)             # (m, ncomp, d)
                A = np.einsum("bad,baf->bdf", J, J)
                w = np.linalg.solve(A[:, None, :, :], gxi[..., None])[..., 0]
                grads[ok] = np.einsum("bad,bcd->bca", J, w)
        return (vals, grads) if gradient else vals

    def dudxi(self, z, elements=None, xi=None):
        """(M, ncomp): sum over the axes and the element's nodes of |dphi_i / dxi| |z_i|, the change of a value per unit
        change of xi (0 where the element is -1)."""
        elem = self.elements if elements is None else np.asarray(elements)
        xi = self.xi if xi is None else np.asarray(xi, dtype=np.float64)
        Z = np.asarray(z, dtype=np.float64)
        Z = Z.reshape(Z.shape[0], -1)
        out = np.zeros((elem.shape[0], Z.shape[1]))
        ok = elem >= 0
        if ok.any():
            _, dphi, _, rows = self._at(elem[ok], xi[ok])
            out[ok] = np.einsum("bdp,bpc->bc", np.abs(dphi), np.abs(Z[rows]))
        return out

    def tol_xi(self, elements=None, xi=None):
        """(M,): max(1e-10, 4 ROUND_FACTOR EPS max|x| |(J^T J)^-1 J^T|_inf) at (elements, xi) (1e-10 where there is none)."""
        elem = self.elements if elements is None else np.asarray(elements)
        xi = self.xi if xi is None else np.asarray(xi, dtype=np.float64)
        out = np.full(elem.shape[0], 1e-10)
        ok = elem >= 0
        if ok.any():
            _, dphi, X, _ = self._at(elem[ok], xi[ok])
            ninv, _, _ = _pinv_norm(np.einsum("bdp,bpa->bad", dphi, X - X[:, :1]))
            xs = np.abs(X).reshape(X.shape[0], -1).max(axis=1)
            out[ok] = np.maximum(1e-10, 4.0 * ROUND_FACTOR * EPS * xs * np.where(np.isfinite(ninv), ninv, 0.0))
        return out

    def tied(self, q, width=1e-9):
        """The elements of point q within `width` of its best distance."""
        dq = self.all_distances[q]
        return np.nonzero(dq - dq.min() < width)[0]


def closest_twin(geom, t, max_distance=None, maxit=TWIN_MAXIT) -> TwinClosest:
    p, N, e = geom.x.shape
    k = geom.discretization.k
    d = geom.discretization.d
    nodes = _tf_nodes(k)
    T = np.asarray(t, dtype=np.float64).reshape(-1, e)
    M = T.shape[0]
    md = default_max_distance(geom) if max_distance is None else float(max_distance)
    Xn = np.asarray(geom.xflat, dtype=np.float64).reshape(N, p, e)
    fin = np.isfinite(T).all(axis=1)
    Tq = np.where(fin[:, None], T, 0.0)
    Xe = np.broadcast_to(Xn[None], (M, N, p, e)).reshape(M * N, p, e)
    q = np.broadcast_to(Tq[:, None, :], (M, N, e)).reshape(M * N, e)
    xi, foot, d2, conv, its = project(Xe, q, nodes, maxit)
    xi, foot, d2 = xi.reshape(M, N, d), foot.reshape(M, N, e), d2.reshape(M, N)
    conv, its = conv.reshape(M, N), its.reshape(M, N)
    dist = np.sqrt(d2)
    best = np.argmin(d2, axis=1)                                       # the first (lowest element) on a tie
    ar = np.arange(M)
    bd = dist[ar, best]
    if N > 1:
        margin = np.sort(dist, axis=1)[:, 1] - bd
    else:
        margin = np.full(M, np.inf)
    ok = fin & (bd <= md)
    elements = np.where(ok, best, -1).astype(np.int32)
    nan = np.nan
    return TwinClosest(geom, nodes, md, elements,
                       np.where(ok[:, None], xi[ar, best], nan), np.where(ok[:, None], foot[ar, best], nan),
                       np.where(ok, bd, nan), conv[ar, best] & ok, margin, xi, foot, dist, conv, its)
