"""NumPy twin of the element quadrature (csrc/quadrature.hip) and a 50-digit evaluation of the same discrete sums.

Both take the float64 tables the device is handed (`mgb_amd.integrate.reference_rule`): the node coordinates `x`
`(p, N, e)`, the reference weights `w` `(Q,)` and the basis at the rule's points `phi` `(Q, p)`, `dphi` `(Q, p, d)`.

    x_q = sum_i phi[q, i] x_i,   J = sum_i x_i dphi[q, i]^T (e x d),   g = J^T J,   measure_q = w_q sqrt(det g),
    u_q = sum_i phi[q, i] z_i,   grad u = J g^-1 xi,   xi = sum_i dphi[q, i] z_i.

`Twin` is plain float64 NumPy.  `Exact` evaluates the sums with mpmath at 50 digits from the same float64 inputs, so its
value is the exact value of what the kernel computes up to 1e-50, and next to every integral it returns `A`, the
integral of a majorant of what a rounding error in the integrand is proportional to (see `Exact.integrate`).
"""
from fractions import Fraction
import math

import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50


def tables(geom, order=None, rule="gauss"):
    """(x (p, N, e), reference rule dict) of a geometry: what `Quadrature(geom, order, rule)` hands the device."""
    import sys
    import mgb_amd.integrate  # noqa: F401  (the package exports a function of the same name)
    ref = sys.modules["mgb_amd.integrate"].reference_rule(geom, order, rule)
    return np.asarray(geom.x, dtype=np.float64), ref


def _cols(Z):
    Z = np.asarray(Z, dtype=np.float64)
    return Z.reshape(Z.shape[0], -1)


class Twin:
    def __init__(self, x, ref):
        self.x = x
        self.p, self.N, self.e = x.shape
        self.w, self.phi, self.dphi = ref["w"], ref["phi"], ref["dphi"]
        self.Q, _, self.d = self.dphi.shape
        self.points = np.einsum("qi,ina->nqa", self.phi, x)                       # (N, Q, e)
        self.J = np.einsum("qib,ina->nqab", self.dphi, x)                         # (N, Q, e, d)
        self.g = np.einsum("nqab,nqac->nqbc", self.J, self.J)
        self.ginv = np.linalg.inv(self.g)
        self.sdet = np.sqrt(np.linalg.det(self.g))
        self.weights = self.w[None, :] * self.sdet                                # (N, Q)

    def kappa(self):
        """(kappa_J, kappa_g): the largest |J|_F |J|abs,F |g^-1|_2 and the largest cond_2(g) over the points, with
        |J|abs = sum_i |x_i| |dphi_i|^T.  What the rounding of J and the closed-form inverse of g are magnified by."""
        Jabs = np.einsum("qib,ina->nqab", np.abs(self.dphi), np.abs(self.x))
        nJ, nJabs = np.sqrt((self.J ** 2).sum(axis=(2, 3))), np.sqrt((Jabs ** 2).sum(axis=(2, 3)))
        gi = np.linalg.norm(self.ginv, 2, axis=(2, 3))
        return float((nJ * nJabs * gi).max()), float((np.linalg.norm(self.g, 2, axis=(2, 3)) * gi).max())

    def fields(self, Z):
        """u (N, Q, ncol) and grad u (N, Q, ncol, e)."""
        Ze = _cols(Z).reshape(self.N, self.p, -1)
        u = np.einsum("qi,nic->nqc", self.phi, Ze)
        xi = np.einsum("qib,nic->nqcb", self.dphi, Ze)
        grad = np.einsum("nqab,nqbd,nqcd->nqca", self.J, self.ginv, xi)
        return u, grad

    def integrand(self, Z, kind, p=2.0, minus=None, source=None):
        """F at the points, (N, Q, ncol); with p = inf the quantity whose maximum norm() returns."""
        u, grad = self.fields(Z)
        ncol = u.shape[2]
        if kind == "value":
            return u
        if kind == "lp":
            v = np.abs(u if minus is None else u - np.asarray(minus, dtype=np.float64).reshape(self.N, self.Q, -1))
            return v if p == math.inf else v ** p
        if kind == "w1p":
            r = grad if minus is None else grad - np.asarray(minus, dtype=np.float64)[:, :, None, :]
            nr = np.sqrt((r * r).sum(axis=3))
            return nr if p == math.inf else nr ** p
        f = np.einsum("qi,ni->nq", self.phi, np.asarray(source, dtype=np.float64).reshape(self.N, self.p))
        return np.sqrt((grad * grad).sum(axis=3)) ** p / p - f[:, :, None] * u + np.zeros((1, 1, ncol))

    def integrate(self, Z, kind, p=2.0, minus=None, source=None):
        """(totals (ncol,), element values (N, ncol)) in float64, every sum by math.fsum."""
        T = self.weights[:, :, None] * self.integrand(Z, kind, p, minus, source)
        elem = np.array([[math.fsum(T[n, :, c]) for c in range(T.shape[2])] for n in range(self.N)])
        return np.array([math.fsum(elem[:, c]) for c in range(elem.shape[1])]), elem

    def u_fused(self, Z):
        """u (N, Q, ncol) exactly as the device forms it: a chain of fused multiply-adds in node order from 0.0, each
        rounded once (Fraction arithmetic is exact and float() rounds to nearest even)."""
        Ze = _cols(Z).reshape(self.N, self.p, -1)
        out = np.zeros((self.N, self.Q, Ze.shape[2]))
        ph = [[Fraction(float(v)) for v in row] for row in self.phi]
        for n in range(self.N):
            for c in range(Ze.shape[2]):
                zc = [Fraction(float(v)) for v in Ze[n, :, c]]
                for q in range(self.Q):
                    acc = 0.0
                    for i in range(self.p):
                        acc = float(ph[q][i] * zc[i] + Fraction(acc))
                    out[n, q, c] = acc
        return out


class Exact:
    """The same sums at 50 digits.  The geometry is formed once; `fields` per (Z, source)."""

    def __init__(self, twin: Twin):
        t = self.t = twin
        mpf = MP.mpf
        N, Q, p, d, e = t.N, t.Q, t.p, t.d, t.e
        self.phi = [[mpf(float(v)) for v in row] for row in t.phi]
        self.dphi = [[[mpf(float(v)) for v in nd] for nd in row] for row in t.dphi]
        self.nzphi = [[i for i in range(p) if t.phi[q, i] != 0.0] for q in range(Q)]
        self.nzd = [[i for i in range(p) if np.any(t.dphi[q, i] != 0.0)] for q in range(Q)]
        x = [[[mpf(float(v)) for v in t.x[i, n]] for i in range(p)] for n in range(N)]
        self.J, self.ginv, self.meas = {}, {}, {}
        for n in range(N):
            for q in range(Q):
                J = MP.matrix(e, d)
                for i in self.nzd[q]:
                    for a in range(e):
                        for b in range(d):
                            J[a, b] += self.dphi[q][i][b] * x[n][i][a]
                g = J.T * J
                self.J[n, q] = J
                self.ginv[n, q] = g ** -1
                self.meas[n, q] = mpf(float(t.w[q])) * MP.sqrt(MP.det(g))
        # float64 is plenty for the factors of A
        Jabs = np.einsum("qib,ina->nqab", np.abs(t.dphi), np.abs(t.x))
        self.jabs = np.sqrt((Jabs ** 2).sum(axis=(2, 3)))                          # |J|abs,F
        self.sigma = np.sqrt(np.linalg.norm(t.ginv, 2, axis=(2, 3)))               # |J g^-1|_2 = 1 / sigma_min(J)

    def fields(self, Z, source=None):
        t, mpf = self.t, MP.mpf
        Ze = _cols(Z).reshape(t.N, t.p, -1)
        ncol = Ze.shape[2]
        u, grad = {}, {}
        for n in range(t.N):
            for c in range(ncol):
                zc = [mpf(float(v)) for v in Ze[n, :, c]]
                for q in range(t.Q):
                    u[n, q, c] = MP.fsum(self.phi[q][i] * zc[i] for i in self.nzphi[q])
                    xi = MP.matrix(t.d, 1)
                    for i in self.nzd[q]:
                        for b in range(t.d):
                            xi[b] += self.dphi[q][i][b] * zc[i]
                    grad[n, q, c] = self.J[n, q] * (self.ginv[n, q] * xi)
        uabs = np.einsum("qi,nic->nqc", np.abs(t.phi), np.abs(Ze))
        xiabs = np.sqrt((np.einsum("qib,nic->nqcb", np.abs(t.dphi), np.abs(Ze)) ** 2).sum(axis=3))
        rho = np.sqrt((np.einsum("nqbd,qid,nic->nqcb", t.ginv, t.dphi, Ze) ** 2).sum(axis=3))      # |g^-1 xi|_2
        gabs = self.jabs[:, :, None] * rho + self.sigma[:, :, None] * xiabs
        out = dict(u=u, grad=grad, uabs=uabs, gabs=gabs, ncol=ncol)
        if source is not None:
            F = np.asarray(source, dtype=np.float64).reshape(t.N, t.p)
            out["f"] = {(n, q): MP.fsum(self.phi[q][i] * mpf(float(F[n, i])) for i in self.nzphi[q])
                        for n in range(t.N) for q in range(t.Q)}
            out["fabs"] = np.einsum("qi,ni->nq", np.abs(t.phi), np.abs(F))
        return out

    def integrate(self, fld, kind, p=2.0, minus=None):
        """(totals, A, element values) per column as lists of mpf (A: floats).

        A is the integral, with the measure as it is, of a majorant of the integrand's sensitivity.  With
        U = sum_i |phi_i z_i| (a rounding error of u_q is a multiple of u U) and
        T = |J|abs,F |g^-1 xi|_2 + |J g^-1|_2 |sum_i |dphi_i| |z_i||_2 (the same for grad u = J g^-1 xi: the first term
        takes the rounding of J, |J|abs = sum_i |x_i| |dphi_i|^T, the second that of xi; T >= |grad u|), and
        m(a, V) = (a + 1e-3 V)^(p-1) V, which bounds | |a + d|^p - |a|^p | / (p |d| / V) for every |d| <= 1e-3 V and
        p >= 1 (mean value theorem):
            value: U;   lp: m(|u - g|, U + |g|);   w1p: m(|grad u - G|, T + |G|_2);
            energy: m(|grad u|, T) + (sum_i |phi_i f_i|) U.
        For p = inf the first return is the maximum over the points and A is None."""
        t, mpf = self.t, MP.mpf
        ncol = fld["ncol"]
        M = None if minus is None else np.asarray(minus, dtype=np.float64)
        if M is not None and kind == "lp":
            M = M.reshape(t.N, t.Q, -1)
        totals, As, elems = [], [], []

        def major(a, V):
            return (a + 1e-3 * V) ** (p - 1.0) * V

        for c in range(ncol):
            ev, av, mx = [], 0.0, mpf(0)
            for n in range(t.N):
                acc = mpf(0)
                for q in range(t.Q):
                    m = self.meas[n, q]
                    if kind == "value":
                        F, a = fld["u"][n, q, c], fld["uabs"][n, q, c]
                    elif kind == "lp":
                        gq = 0.0 if M is None else float(M[n, q, c if M.shape[2] > 1 else 0])
                        v = abs(fld["u"][n, q, c] - mpf(gq))
                        F = v if p == math.inf else v ** mpf(p)
                        a = 0.0 if p == math.inf else major(float(v), fld["uabs"][n, q, c] + abs(gq))
                    else:
                        r = fld["grad"][n, q, c]
                        Gn = 0.0
                        if kind == "w1p" and M is not None:
                            r = r - MP.matrix([mpf(float(v)) for v in M[n, q]])
                            Gn = float(np.sqrt((M[n, q] ** 2).sum()))
                        nr = MP.sqrt(sum(v * v for v in r))
                        if kind == "w1p":
                            F = nr if p == math.inf else nr ** mpf(p)
                            a = 0.0 if p == math.inf else major(float(nr), fld["gabs"][n, q, c] + Gn)
                        else:
                            F = nr ** mpf(p) / mpf(p) - fld["f"][n, q] * fld["u"][n, q, c]
                            a = major(float(nr), fld["gabs"][n, q, c]) + fld["fabs"][n, q] * fld["uabs"][n, q, c]
                    if p == math.inf:
                        mx = max(mx, F)
                    else:
                        acc += m * F
                        av += abs(float(m)) * a
                ev.append(acc)
            if p == math.inf:
                totals.append(mx)
                As.append(None)
            else:
                totals.append(MP.fsum(ev))
                As.append(av)
            elems.append(ev)
        return totals, As, elems
