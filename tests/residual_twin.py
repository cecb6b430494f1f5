"""A 50-digit evaluation of the element residual (csrc/residual.hip) from the float64 tables the device is handed
(`mgb_amd.estimate.residual_tables`): the node coordinates `x` `(p, N, d)`, the reference weights `w` `(Q,)` and the basis
at the rule's points `phi` `(Q, p)`, `dphi` `(Q, p, d)`, `d2phi` `(Q, p, d(d+1)/2)`.

    J = sum_i x_i dphi[q, i]^T,   measure_q = w_q det J,   g = grad u = J^-T sum_i dphi[q, i] z_i,
    H_xi(v)[b][c] = sum_i v_i d2phi[q, i, (b, c)],   H = J^-T ( H_xi(z) - sum_a g_a H_xi(x_a) ) J^-1,
    div a = |g|^(p-2) ( tr H + (p - 2) g^T H g / |g|^2 )   (p = 2: tr H;  g = 0 and p != 2: 0),   r_q = f_q + div a,
    h_K = (sum_q measure_q)^(1/d),   interior_K = h_K^2 sum_q measure_q r_q^2.

`Exact` forms the physical Hessian `H` as written here (the kernel never forms it: it takes the trace and the quadratic
form through `(J^T J)^-1` and `J^-1 g`), with mpmath at 50 digits, so its values are those of what the kernel computes up
to 1e-50.  Next to every value it returns `A`, a majorant of what a rounding error is proportional to (`Exact.residual`).
The face half of the estimator is `faces_twin.Exact`; `indicator` below gathers its jumps as `Faces.indicator` does.
"""
import math

import mpmath
import numpy as np

from integrate_twin import _cols

MP = mpmath.mp.clone()
MP.dps = 50


def tables(geom, order=None):
    """(x (p, N, d), tables dict) of a geometry: what `ResidualEstimator(geom, order)` hands the device."""
    import sys
    import mgb_amd.estimate  # noqa: F401
    return np.asarray(geom.x, dtype=np.float64), sys.modules["mgb_amd.estimate"].residual_tables(geom, order)


def _full(d, v):
    """The symmetric d x d array of the d(d+1)/2 entries v[..., m] in the tables' order."""
    out = np.zeros(v.shape[:-1] + (d, d))
    m = 0
    for b in range(d):
        for c in range(b, d):
            out[..., b, c] = out[..., c, b] = v[..., m]
            m += 1
    return out


class Exact:
    """The element residual at 50 digits.  The geometry is formed once; `fields` per (Z, source); `residual` and
    `interior` per exponent."""

    def __init__(self, x, tb):
        mpf = MP.mpf
        self.x = x = np.asarray(x, dtype=np.float64)
        self.p, self.N, self.d = x.shape
        self.w, self.phi, self.dphi, self.d2phi = tb["w"], tb["phi"], tb["dphi"], tb["d2phi"]
        self.Q = self.phi.shape[0]
        p, N, d, Q = self.p, self.N, self.d, self.Q
        self.pairs = [(b, c) for b in range(d) for c in range(b, d)]
        self.mphi = [[mpf(float(v)) for v in row] for row in self.phi]
        self.mdphi = [[[mpf(float(v)) for v in nd] for nd in row] for row in self.dphi]
        self.md2 = [[[mpf(float(v)) for v in nd] for nd in row] for row in self.d2phi]
        self.nz2 = [[i for i in range(p) if np.any(self.d2phi[q, i] != 0.0)] for q in range(Q)]
        self.mx = [[[mpf(float(v)) for v in x[i, n]] for i in range(p)] for n in range(N)]
        self.Ji, self.det, self.meas, self.Hx = {}, {}, {}, {}
        for n in range(N):
            for q in range(Q):
                J = MP.matrix(d, d)
                for i in range(p):
                    for a in range(d):
                        for b in range(d):
                            J[a, b] += self.mdphi[q][i][b] * self.mx[n][i][a]
                self.Ji[n, q] = J ** -1
                self.det[n, q] = MP.det(J)
                self.meas[n, q] = mpf(float(self.w[q])) * self.det[n, q]
                self.Hx[n, q] = [self.hessian_xi(q, [self.mx[n][i][a] for i in range(p)]) for a in range(d)]
        # float64 is plenty for the factors of A and of the constants
        Jf = np.einsum("qib,ina->nqab", self.dphi, x)
        Jabs = np.einsum("qib,ina->nqab", np.abs(self.dphi), np.abs(x))
        sv = np.linalg.svd(Jf, compute_uv=False)                                   # (N, Q, d), descending
        self.sigma = 1.0 / sv[..., -1]                                             # |J^-1|_2
        self.jabs = np.sqrt((Jabs ** 2).sum(axis=(2, 3)))                          # |J|abs,F
        self.kJ = float((self.sigma * self.jabs).max())
        self.kappa = float((sv[..., 0] / sv[..., -1]).max())
        self.GiF = np.linalg.norm(np.linalg.inv(np.einsum("nqab,nqac->nqbc", Jf, Jf)), "fro", axis=(2, 3))
        Hxabs = _full(d, np.einsum("qim,ina->nqam", np.abs(self.d2phi), np.abs(x)))        # (N, Q, d, d, d)
        self.HxabsF = np.sqrt((Hxabs ** 2).sum(axis=(2, 3, 4)))
        self.rho = 1.0         # the largest T / |grad u| seen by `fields`

    def hessian_xi(self, q, v):
        """H_xi(v) at point q as an mp matrix, v the p nodal values as mpf."""
        d = self.d
        H = MP.matrix(d, d)
        for m, (b, c) in enumerate(self.pairs):
            s = MP.fsum(self.md2[q][i][m] * v[i] for i in self.nz2[q])
            H[b, c] = s
            H[c, b] = s
        return H

    def sizes(self):
        """h_K as mpf, one per element."""
        return [MP.root(MP.fsum(self.meas[n, q] for q in range(self.Q)), self.d) for n in range(self.N)]

    def fields(self, Z, source):
        """Per (element, point, column): grad u and the physical Hessian H (mp), and the floats `T` (an error of grad u
        is a multiple of u T, `faces_twin.Exact._side` without the shift by z_0) and `Mm = |sum_i |d2phi_i| |z_i||_F +
        T (sum_a |sum_i |d2phi_i| |x_i,a||_F^2)^(1/2)`, which bounds |H_xi(z) - sum_a g_a H_xi(x_a)|_F and what its
        rounding errors are proportional to.  `f` per (element, point) with `fabs = sum_i |phi_i f_i|`, or `|f_q|` for a
        source given at the points."""
        mpf, d, p, N, Q = MP.mpf, self.d, self.p, self.N, self.Q
        Ze = _cols(Z).reshape(N, p, -1)
        ncol = Ze.shape[2]
        g, H = {}, {}
        for n in range(N):
            for c in range(ncol):
                zc = [mpf(float(v)) for v in Ze[n, :, c]]
                for q in range(Q):
                    xi = MP.matrix(d, 1)
                    for i in range(p):
                        for b in range(d):
                            xi[b] += self.mdphi[q][i][b] * zc[i]
                    Ji = self.Ji[n, q]
                    gg = Ji.T * xi
                    M = self.hessian_xi(q, zc)
                    for a in range(d):
                        M = M - gg[a] * self.Hx[n, q][a]
                    g[n, q, c] = gg
                    H[n, q, c] = Ji.T * M * Ji
        xiabs = np.sqrt((np.einsum("qib,nic->nqcb", np.abs(self.dphi), np.abs(Ze)) ** 2).sum(axis=3))
        gn = np.array([[[float(MP.sqrt(sum(v * v for v in g[n, q, c]))) for c in range(ncol)] for q in range(Q)]
                       for n in range(N)])
        T = self.sigma[:, :, None] * (self.jabs[:, :, None] * gn + xiabs)
        Hzabs = _full(d, np.einsum("qim,nic->nqcm", np.abs(self.d2phi), np.abs(Ze)))
        Mm = np.sqrt((Hzabs ** 2).sum(axis=(3, 4))) + T * self.HxabsF[:, :, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(gn > 0, T / gn, 1.0)
        self.rho = max(self.rho, float(rho.max()))
        return dict(g=g, H=H, gn=gn, T=T, Mm=Mm, ncol=ncol, **self.source(source))

    def source(self, source):
        """`f` (mpf) and `fabs` (float) per (element, point) of a source in either form: the entries of `fields` that
        depend on it (`dict(fld, **ex.source(other))` swaps the source of a field set)."""
        mpf, p, N, Q = MP.mpf, self.p, self.N, self.Q
        F = np.asarray(source, dtype=np.float64)
        if F.ndim == 1:
            Fe = F.reshape(N, p)
            f = {(n, q): MP.fsum(self.mphi[q][i] * mpf(float(Fe[n, i])) for i in range(p)) for n in range(N) for q in range(Q)}
            fabs = np.einsum("qi,ni->nq", np.abs(self.phi), np.abs(Fe))
        else:
            f = {(n, q): mpf(float(F[n, q])) for n in range(N) for q in range(Q)}
            fabs = np.abs(F)
        return dict(f=f, fabs=fabs)

    def residual(self, fld, p):
        """(r, A): dicts over (element, point, column) of the strong residual (mpf) and of its majorant (float),
        A = fabs + (1 + |p - 2|) G |(J^T J)^-1|_F Mm >= |f| + |div a| with G = 1 for p = 2, (|g| + 1e-3 T)^(p-2) for
        p > 2 and (|g| - 1e-3 T)^(p-2) for p < 2 (the power at the worst gradient within its own rounding error, as in
        `faces_twin.Exact.majorant`; p < 2 needs |g| >= 2e-3 T, asserted).  tr H = sum M_bc (J^T J)^-1_bc and
        g^T H g / |g|^2 are both at most |(J^T J)^-1|_F |M|_F."""
        d, mp2 = self.d, MP.mpf(p) - 2
        r, A = {}, {}
        for (n, q, c), H in fld["H"].items():
            g, gn, T = fld["g"][n, q, c], fld["gn"][n, q, c], fld["T"][n, q, c]
            tr = sum(H[a, a] for a in range(d))
            if p == 2.0:
                diva, G = tr, 1.0
            elif gn == 0.0:
                diva, G = MP.mpf(0), 0.0
            else:
                s2 = sum(v * v for v in g)
                gHg = sum(g[a] * H[a, b] * g[b] for a in range(d) for b in range(d))
                diva = s2 ** (mp2 / 2) * (tr + mp2 * gHg / s2)
                if p > 2.0:
                    G = (gn + 1e-3 * T) ** (p - 2.0)
                else:
                    assert gn >= 2e-3 * T, ("the gradient is too small against its rounding error for a first-order bound", gn, T)
                    G = (gn - 1e-3 * T) ** (p - 2.0)
            r[n, q, c] = fld["f"][n, q] + diva
            A[n, q, c] = fld["fabs"][n, q] + (1.0 + abs(p - 2.0)) * G * self.GiF[n, q] * fld["Mm"][n, q, c]
        return r, A

    def interior(self, fld, p):
        """(values, A, totals, A totals), lists per column: interior_K = h_K^2 sum_q measure_q r_q^2 per element (mpf), the
        same sum of A_q^2 (float: (r + dr)^2 - r^2 = 2 r dr and |r| <= A), and both summed over the elements."""
        r, A = self.residual(fld, p)
        h = self.sizes()
        vals, As = [], []
        for c in range(fld["ncol"]):
            vals.append([h[n] * h[n] * MP.fsum(self.meas[n, q] * r[n, q, c] ** 2 for q in range(self.Q)) for n in range(self.N)])
            As.append([float(h[n] * h[n]) * math.fsum(float(self.meas[n, q]) * A[n, q, c] ** 2 for q in range(self.Q))
                       for n in range(self.N)])
        return vals, As, [MP.fsum(v) for v in vals], [math.fsum(a) for a in As]


def indicator(fex, interior, orientation, element_faces, Z, p, cache=None):
    """(values, A), lists per column over the elements: `Faces.indicator` from `faces_twin.Exact` `fex`: the sum over an
    element's interior faces of (h_F / 2) int_F [flux]^2 with h_F = |F|^(1/(d-1)), and the same gather of the jumps' A."""
    vals, Af = fex.jumps(interior, orientation, Z, "flux", p, cache=cache)
    meas = [[fex.geo(int(r[0]), int(r[1]), q)[2] for q in range(fex.Qf)] for r in interior]
    hF = [MP.root(MP.fsum(m), fex.d - 1) for m in meas]
    N, F = element_faces.shape
    out, outA = [], []
    for c in range(len(vals)):
        ev, ea = [], []
        for n in range(N):
            idx = [int(i) for i in element_faces[n] if i >= 0]
            ev.append(MP.fsum(hF[i] / 2 * vals[c][i] for i in idx))
            ea.append(math.fsum(float(hF[i]) / 2 * Af[c][i] for i in idx))
        out.append(ev)
        outA.append(ea)
    return out, outA


# ---- the cases the CPU and the GPU tests share ---------------------------------------------------------------------

def warp(x, amp=0.06):
    """A smooth map of the nodes (that of tests/test_gpu_integrate.py): elements stay valid and conforming, no element
    map stays affine."""
    y = x.copy()
    s = x.sum(axis=-1)
    for a in range(x.shape[-1]):
        y[..., a] += amp * np.sin(1.3 * s + 0.7 * a) + 0.5 * amp * x[..., (a + 1) % x.shape[-1]] ** 2
    return y


def cases(m):
    """name -> (geometry maker, order): every family of the estimator on a warped mesh of 4 to 16 elements."""
    return {
        "fem2d_k1": (lambda: m.fem2d(k=1, K=warp(m.subdivide(m.fem2d(k=1), 3).x)), None),
        "fem2d_k3": (lambda: m.fem2d(k=3, K=warp(m.subdivide(m.fem2d(k=3), 2).x)), None),
        "fem3d_k2": (lambda: m.fem3d(k=2, K=warp(m.subdivide(m.fem3d(k=2), 2).x, 0.03)), 3),
        "fem2d_P1": (lambda: m.fem2d_P1(K=warp(m.subdivide(m.fem2d_P1(), 2).x)), None),
        "fem2d_P2": (lambda: m.fem2d_P2(K=warp(m.subdivide(m.fem2d_P2(), 2).x), curved=True), None),
        "fem2d_P2_nobubble": (lambda: m.fem2d_P2(bubble=False, K=warp(m.subdivide(m.fem2d_P2(bubble=False), 2).x),
                                                 curved=True), None),
    }


def smooth_u(X):
    """u = 2 x + y (+ 0.5 z) + 0.3 x y + 0.2 x^2 (+ 0.1 y z): its first gradient component is at least 1.3 on [-1, 1]^d."""
    u = 2.0 * X[:, 0] + X[:, 1] + 0.3 * X[:, 0] * X[:, 1] + 0.2 * X[:, 0] ** 2
    if X.shape[1] == 3:
        u = u + 0.5 * X[:, 2] + 0.1 * X[:, 1] * X[:, 2]
    return u


def data(geom, ncol=2):
    """(Z (p*N, ncol), an element-space source (p*N,)): column 0 interpolates `smooth_u`, the others scale it and add a
    small smooth perturbation."""
    X = geom.xflat
    u = smooth_u(X)
    Z = np.stack([u * (1.0 - 0.05 * c) + 0.01 * c * np.sin(3.0 * X[:, 0] + 2.0 * X[:, 1]) for c in range(ncol)], axis=1)
    return Z, np.cos(X[:, 0]) + 0.3 * X[:, 1]


def source_at(points):
    """The same source evaluated at points (N, Q, d): values at the points, (N, Q)."""
    return np.cos(points[..., 0]) + 0.3 * points[..., 1]


def gradient_norms(x, tb, Z):
    """|grad u| (N, Q, ncol) in float64 NumPy: what the p != 2 cases rely on staying away from 0."""
    p, N, d = x.shape
    J = np.einsum("qib,ina->nqab", tb["dphi"], x)
    xi = np.einsum("qib,nic->nqcb", tb["dphi"], _cols(Z).reshape(N, p, -1))
    g = np.einsum("nqba,nqcb->nqca", np.linalg.inv(J), xi)
    return np.sqrt((g * g).sum(axis=3))
