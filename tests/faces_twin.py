"""Twin of the face code (csrc/faces.hip): the topology as a dict over sorted id tuples, and a 50-digit evaluation of the
face integrals from the float64 tables the device is handed (`mgb_amd.faces.face_tables`).

At point q of local face f of an element with nodes x_i and values z_i

    J = sum_i x_i dphi[f, q, i]^T,   grad u = J^-T sum_i z_i dphi[f, q, i],   n = J^-T n_ref / |J^-T n_ref|,
    ds = wf_q |J t| (2-D) or wf_q |J t1 x J t2| (3-D),   a = |grad u|^(p-2) grad u  (0 where grad u = 0).

`Exact` evaluates these with mpmath at 50 digits, so its values are those of what the kernel computes up to 1e-50, and
next to every integral it returns `A`: the face measure times a majorant of what a rounding error of the integrand is
proportional to (see `Exact.majorant`).
"""
import mpmath
import numpy as np

MP = mpmath.mp.clone()
MP.dps = 50


def topology(t, corners):
    """boundary (B, 2), interior (I, 4), orientation (I,), element_faces (N, F) of the connectivity `t` (p, N) with the
    local face corners `corners` (F, NC), from a dict over the sorted tuples of *all* corner ids of a face.  ValueError
    naming the count if more than two elements share a face."""
    t = np.asarray(t)
    N, F, NC = t.shape[1], corners.shape[0], corners.shape[1]
    seen = {}
    for e in range(N):
        for f in range(F):
            seen.setdefault(tuple(sorted(int(t[c, e]) for c in corners[f])), []).append((e, f))
    most = max(len(v) for v in seen.values())
    if most > 2:
        raise ValueError(f"a face is shared by {most} elements")
    boundary = sorted(v[0] for v in seen.values() if len(v) == 1)
    interior = sorted(v[0] + v[1] for v in seen.values() if len(v) == 2)        # v[0] < v[1]: the loop above ascends
    orientation = []
    for eL, fL, eR, fR in interior:
        idsL = [int(t[c, eL]) for c in corners[fL]]
        idsR = [int(t[c, eR]) for c in corners[fR]]
        i0, i1 = idsR.index(idsL[0]), idsR.index(idsL[1])
        orientation.append(i0 if NC == 2 else 2 * i0 + {1: 0, 2: 1}[i0 ^ i1])
    ef = np.zeros((N, F), dtype=np.int32)
    for b, (e, f) in enumerate(boundary):
        ef[e, f] = -1 - b
    for i, (eL, fL, eR, fR) in enumerate(interior):
        ef[eL, fL] = ef[eR, fR] = i
    return (np.array(boundary, dtype=np.int32).reshape(-1, 2), np.array(interior, dtype=np.int32).reshape(-1, 4),
            np.array(orientation, dtype=np.int32), ef)


def _cols(Z):
    Z = np.asarray(Z, dtype=np.float64)
    return Z.reshape(Z.shape[0], -1)


class Exact:
    """The face quantities at 50 digits.  `x` (p, N, d) node coordinates, `tb` the tables of `face_tables`."""

    def __init__(self, x, tb):
        self.x, self.tb = np.asarray(x, dtype=np.float64), tb
        self.p, self.N, self.d = self.x.shape
        self.F, self.Qf = tb["xi"].shape[:2]
        self._geo = {}
        self.kJ = 0.0          # the largest |J^-1|_2 |J|abs,F seen, |J|abs = sum_i |x_i| |dphi_i|^T
        self.kappa = 0.0       # the largest cond_2(J) seen

    def geo(self, e, f, q):
        """(J^-T as an mp matrix, unit normal as an mp column, ds as mpf, x_q as floats, sigma = |J^-1|_2, |J|abs,F, det J)."""
        key = (e, f, q)
        if key not in self._geo:
            mpf, d, tb = MP.mpf, self.d, self.tb
            J = MP.matrix(d, d)
            for i in range(self.p):
                dp = tb["dphi"][f, q, i]
                if np.any(dp != 0.0):
                    for a in range(d):
                        xa = mpf(float(self.x[i, e, a]))
                        for b in range(d):
                            J[a, b] += xa * mpf(float(dp[b]))
            JiT = (J ** -1).T
            nr = JiT * MP.matrix([mpf(float(v)) for v in tb["normals"][f]])
            n = nr / MP.sqrt(sum(v * v for v in nr))
            tang = [J * MP.matrix([mpf(float(v)) for v in tb["tangents"][f, j]]) for j in range(d - 1)]
            if d == 2:
                ln = MP.sqrt(sum(v * v for v in tang[0]))
            else:
                u, v = tang
                cr = [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
                ln = MP.sqrt(sum(c * c for c in cr))
            ds = mpf(float(tb["wf"][q])) * ln
            Jf = np.einsum("ib,ia->ab", tb["dphi"][f, q], self.x[:, e, :])
            Jabs = np.einsum("ib,ia->ab", np.abs(tb["dphi"][f, q]), np.abs(self.x[:, e, :]))
            sv = np.linalg.svd(Jf, compute_uv=False)
            sigma, jabs = 1.0 / sv[-1], float(np.sqrt((Jabs ** 2).sum()))
            self.kJ, self.kappa = max(self.kJ, sigma * jabs), max(self.kappa, sv[0] / sv[-1])
            xq = tb["phi"][f, q] @ self.x[:, e, :]
            self._geo[key] = (JiT, n, ds, xq, sigma, jabs, float(MP.det(J)))
        return self._geo[key]

    def side(self, Ze, e, f, q, cache=None):
        """`_side`, kept in `cache` (a dict the caller holds per Z) so that the kinds and exponents share it."""
        if cache is None:
            return self._side(Ze, e, f, q)
        if (e, f, q) not in cache:
            cache[e, f, q] = self._side(Ze, e, f, q)
        return cache[e, f, q]

    def _side(self, Ze, e, f, q):
        """Per column of Ze (N, p, ncol): u, grad u (mp), and the floats U = sum_i |phi_i z_i| and
        T = |J^-1|_2 (|J|abs,F |grad u| + |sum_i |dphi_i| |z_i - z_0||_2) >= |grad u|: a rounding error of u is a multiple
        of u U, one of grad u a multiple of u T (the first term takes the rounding of J, the second that of the sum, which
        the kernel forms from the differences z_i - z_0: the dphi_i sum to zero)."""
        JiT, n, ds, _, sigma, jabs, _ = self.geo(e, f, q)
        mpf, d, tb = MP.mpf, self.d, self.tb
        out = []
        for c in range(Ze.shape[2]):
            z = Ze[e, :, c]
            u = MP.fsum(mpf(float(tb["phi"][f, q, i])) * mpf(float(z[i])) for i in range(self.p) if tb["phi"][f, q, i] != 0.0)
            xi = MP.matrix(d, 1)
            for i in range(self.p):
                for b in range(d):
                    xi[b] += mpf(float(tb["dphi"][f, q, i, b])) * mpf(float(z[i]))
            g = JiT * xi
            gn = float(MP.sqrt(sum(v * v for v in g)))
            U = float(np.abs(tb["phi"][f, q] * z).sum())
            xiabs = float(np.sqrt(((np.abs(tb["dphi"][f, q]) * np.abs(z - z[0])[:, None]).sum(axis=0) ** 2).sum()))
            out.append((u, g, U, sigma * (jabs * gn + xiabs)))
        return out

    @staticmethod
    def flux(g, n, p):
        """a(g) . n = |g|^(p-2) g . n, 0 at g = 0."""
        s2 = sum(v * v for v in g)
        if s2 == 0:
            return MP.mpf(0)
        return s2 ** ((MP.mpf(p) - 2) / 2) * sum(a * b for a, b in zip(g, n))

    @staticmethod
    def majorant(g, T, p):
        """What a rounding error of a(g) . n is proportional to: |da| <= max(1, p - 1) |g~|^(p-2) |dg| at some g~ between,
        |dg| a multiple of u T, and the rounding of n and of the products moves a . n by multiples of u |a|,
        |a| = |g|^(p-1) <= |g|^(p-2) T.  For every |dg| <= 1e-3 T: p >= 2: max(1, p-1) (|g| + 1e-3 T)^(p-2) T;
        1 <= p < 2: (|g| - 1e-3 T)^(p-2) T, which needs |g| >= 2e-3 T (asserted: below that the gradient is lost in its
        own rounding error and a first-order bound says nothing); 0 where T = 0."""
        gn = float(MP.sqrt(sum(v * v for v in g)))
        if T == 0.0:
            return 0.0
        if p >= 2.0:
            return max(1.0, p - 1.0) * (gn + 1e-3 * T) ** (p - 2.0) * T
        assert gn >= 2e-3 * T, ("the gradient is too small against its rounding error for a first-order bound", gn, T)
        return (gn - 1e-3 * T) ** (p - 2.0) * T

    def boundary(self, boundary, Z, kind, p=2.0, weight=None, cache=None):
        """(totals, A totals, face values, A per face), lists per column: the integrals over the boundary faces and, with
        the same measure and |weight|, the integral of U (value) or of the flux majorant."""
        Ze = _cols(Z).reshape(self.N, self.p, -1)
        ncol = Ze.shape[2]
        vals = [[MP.mpf(0)] * len(boundary) for _ in range(ncol)]
        As = [[0.0] * len(boundary) for _ in range(ncol)]
        for b, (e, f) in enumerate(boundary):
            for q in range(self.Qf):
                _, n, ds, _, _, _, _ = self.geo(e, f, q)
                w = 1.0 if weight is None else float(weight[b, q])
                for c, (u, g, U, T) in enumerate(self.side(Ze, e, f, q, cache)):
                    F = u if kind == "value" else self.flux(g, n, p)
                    a = U if kind == "value" else self.majorant(g, T, p)
                    vals[c][b] = vals[c][b] + ds * MP.mpf(w) * F
                    As[c][b] += float(ds) * abs(w) * a
        return [MP.fsum(v) for v in vals], [float(sum(a)) for a in As], vals, As

    def jumps(self, interior, orientation, Z, kind, p=2.0, cache=None):
        """(face values, A per face), lists per column: int (u_L - u_R)^2 resp. int (a_L . n_L + a_R . n_R)^2 with the L
        side's measure; A from (U_L + U_R)^2 resp. (m_L + m_R)^2, m the flux majorant of a side: a difference of nearly
        equal numbers is measured against the numbers it was formed from."""
        Ze = _cols(Z).reshape(self.N, self.p, -1)
        ncol = Ze.shape[2]
        perm = self.tb["perm"]
        vals = [[MP.mpf(0)] * len(interior) for _ in range(ncol)]
        As = [[0.0] * len(interior) for _ in range(ncol)]
        for i, (eL, fL, eR, fR) in enumerate(interior):
            for q in range(self.Qf):
                qR = int(perm[orientation[i], q])
                _, nL, ds, _, _, _, _ = self.geo(eL, fL, q)
                _, nR, _, _, _, _, _ = self.geo(eR, fR, qR)
                sL, sR = self.side(Ze, eL, fL, q, cache), self.side(Ze, eR, fR, qR, cache)
                for c in range(ncol):
                    (uL, gL, UL, TL), (uR, gR, UR, TR) = sL[c], sR[c]
                    if kind == "value":
                        j, a = uL - uR, UL + UR
                    else:
                        j, a = self.flux(gL, nL, p) + self.flux(gR, nR, p), self.majorant(gL, TL, p) + self.majorant(gR, TR, p)
                    vals[c][i] = vals[c][i] + ds * j * j
                    As[c][i] += float(ds) * a * a
        return vals, As

    def measures(self, faces):
        """ds (nf, Qf) as floats, from the first [element, face] of every row."""
        return np.array([[float(self.geo(int(r[0]), int(r[1]), q)[2]) for q in range(self.Qf)] for r in faces]).reshape(-1, self.Qf)
