"""interpolate(..., gradient=True) on the device (-m gpu): an extended-precision host oracle, polynomial reproduction,
central differences of device values, the operators the solver uses, the semantics of the value path, a real solve.

Error measure of sections 1, 2 and 4, per point q: |g_dev - g_ref|_inf / S(q) with S(q) = sum_i |grad_x phi_i(q)|_inf
|z_i| over the local basis functions of the element the device reported: the rounding scale of the sum that is the
gradient (it also absorbs |J^{-1}|).  The admissible multiple of eps is not a constant of this file: next to the
np.longdouble oracle runs a plain float64 NumPy twin of it (float64 Newton for xi with the documented stopping rule
max(1e-13, 64 eps max|x| |J^{-1}|_inf), float64 sums), whose largest ratio against the oracle is measured at run time,
per family; the device is allowed DEVICE_FACTOR = 16 times that (a different summation order; a wrong Jacobian, axis
or sign is off by O(1 / eps)).  The twin itself must stay below TWIN_CAP = 2^10 eps for every family.
"""
import zlib

import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd import fem2d_p1, fem2d_p2
from mgb_amd.interpolate import _spectral1d_coefficients, _spectral2d_coefficients
from mgb_amd.tensorfem import _tf_nodes
from test_gpu_interpolate import REPRO, SHIFTED, _interior, _repro_geom

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
DEVICE_FACTOR = 16.0
TWIN_CAP = 2.0 ** 10 * EPS


# ---------------------------------------------------------------------------------------------------------------------
# host evaluation of grad_x phi_i(q) for every local basis function, in a chosen dtype, from the basis definitions
# ---------------------------------------------------------------------------------------------------------------------

def _inv(J):
    """Inverse of (M, d, d) matrices by cofactors, d = 1, 2, 3, in J's dtype; also |J^{-1}|_inf."""
    d = J.shape[1]
    Ji = np.empty_like(J)
    if d == 1:
        Ji[:, 0, 0] = 1 / J[:, 0, 0]
    elif d == 2:
        det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
        Ji[:, 0, 0], Ji[:, 0, 1] = J[:, 1, 1] / det, -J[:, 0, 1] / det
        Ji[:, 1, 0], Ji[:, 1, 1] = -J[:, 1, 0] / det, J[:, 0, 0] / det
    else:
        c = np.empty_like(J)
        for a in range(3):
            for b in range(3):
                r = [i for i in range(3) if i != a]
                s = [i for i in range(3) if i != b]
                c[:, a, b] = (-1) ** (a + b) * (J[:, r[0], s[0]] * J[:, r[1], s[1]] - J[:, r[0], s[1]] * J[:, r[1], s[0]])
        det = J[:, 0, 0] * c[:, 0, 0] + J[:, 0, 1] * c[:, 0, 1] + J[:, 0, 2] * c[:, 0, 2]
        Ji = c.transpose(0, 2, 1) / det[:, None, None]
    return Ji, np.abs(Ji).sum(axis=2).max(axis=1)


def _lagrange_all(nodes, X):
    """L_i and L_i' of the 1-D Lagrange basis on `nodes` at X (any shape): arrays X.shape + (S,)."""
    S = len(nodes)
    L = np.empty(X.shape + (S,), dtype=X.dtype)
    dL = np.empty_like(L)
    for i in range(S):
        den = np.prod([nodes[i] - nodes[j] for j in range(S) if j != i], dtype=X.dtype)
        num = np.ones_like(X)
        for j in range(S):
            if j != i:
                num = num * (X - nodes[j])
        dnum = np.zeros_like(X)
        for mm in range(S):
            if mm != i:
                t = np.ones_like(X)
                for j in range(S):
                    if j != i and j != mm:
                        t = t * (X - nodes[j])
                dnum = dnum + t
        L[..., i] = num / den
        dL[..., i] = dnum / den
    return L, dL


def _tensor(L, dL):
    """phi (M, p) and dphi/dxi (M, p, d) of the tensor basis, local node lin = i0 + S i1 + S^2 i2 (axis 0 fastest)."""
    M, d, S = L.shape
    if d == 1:
        return L[:, 0], dL[:, 0][:, :, None]
    if d == 2:
        phi = L[:, 1, :, None] * L[:, 0, None, :]
        d0 = L[:, 1, :, None] * dL[:, 0, None, :]
        d1 = dL[:, 1, :, None] * L[:, 0, None, :]
        return phi.reshape(M, -1), np.stack([d0.reshape(M, -1), d1.reshape(M, -1)], axis=2)
    f = lambda A2, A1, A0: (A2[:, :, None, None] * A1[:, None, :, None] * A0[:, None, None, :]).reshape(M, -1)
    phi = f(L[:, 2], L[:, 1], L[:, 0])
    return phi, np.stack([f(L[:, 2], L[:, 1], dL[:, 0]), f(L[:, 2], dL[:, 1], L[:, 0]), f(dL[:, 2], L[:, 1], L[:, 0])],
                         axis=2)


def _qk_xi(geom, elem, pts, dtype):
    """Reference coordinates (M, d) of pts[q] in the Q_k element elem[q]: Newton from xi = 0 on the element map.
    longdouble: 40 full steps; float64: the documented stopping rule of the device, 32 steps at most."""
    nodes = _tf_nodes(geom.discretization.k).astype(dtype)
    Xe = geom.x.astype(dtype)[:, elem, :].transpose(1, 0, 2)             # (M, p, d)
    P = pts.astype(dtype)
    M, d = P.shape
    xi = np.zeros((M, d), dtype=dtype)
    done = np.zeros(M, dtype=bool)
    exact = dtype is LD
    xs = np.maximum(np.abs(Xe).max(axis=(1, 2)), np.abs(P).max(axis=1))
    for _ in range(40 if exact else 32):
        L, dL = _lagrange_all(nodes, xi)
        phi, dphi = _tensor(L, dL)
        F = np.einsum("mp,mpa->ma", phi, Xe) - P
        J = np.einsum("mpb,mpa->mab", dphi, Xe)
        Ji, ninv = _inv(J)
        dx = np.einsum("mab,mb->ma", Ji, F)
        xi = np.where(done[:, None], xi, xi - dx)
        if not exact:
            done |= np.abs(dx).max(axis=1) <= np.maximum(1e-13, 64 * EPS * xs * ninv)
            if done.all():
                break
    return xi, Xe


def _qk_basis_grads(geom, elem, pts, dtype):
    """(M, p, d) gradients in x of the Q_k basis of element elem[q] at pts[q]: J^{-T} grad_xi phi_i at the located xi."""
    xi, Xe = _qk_xi(geom, elem, pts, dtype)
    L, dL = _lagrange_all(_tf_nodes(geom.discretization.k).astype(dtype), xi)
    _, dphi = _tensor(L, dL)
    Ji, _ = _inv(np.einsum("mpb,mpa->mab", dphi, Xe))
    return np.einsum("mba,mpb->mpa", Ji, dphi)


def _simplex_basis_grads(geom, elem, pts, dtype):
    """(M, p, 2) gradients in x of the P1 / P2 basis: the coefficient table over the monomials l1^i l2^j differentiated,
    mapped by the inverse transpose of the edge vectors (l1 = 1 at the first corner slot, l2 = 1 at the second, the
    third is the origin)."""
    p = geom.x.shape[0]
    if p == 3:
        table, (s0, s1, s2) = fem2d_p1.basis_coefficient_table(), (0, 1, 2)
    else:
        table, (s0, s1, s2) = fem2d_p2.basis_coefficient_table(p == 7), (0, 2, 4)
    T = table.astype(dtype)
    X = geom.x.astype(dtype)[:, elem, :]                                  # (p, M, 2)
    P = pts.astype(dtype)
    J = np.stack([X[s0] - X[s2], X[s1] - X[s2]], axis=2)                  # columns: the two edge vectors
    Ji, _ = _inv(J)
    l = np.einsum("mab,mb->ma", Ji, P - X[s2])
    l1, l2 = l[:, 0], l[:, 1]
    one = np.ones_like(l1)
    pw = lambda v, e: one if e == 0 else v ** e
    d1 = np.stack([(i * pw(l1, i - 1) * pw(l2, j)) if i > 0 else 0 * one for i, j in fem2d_p2.MONOMIALS], axis=1)
    d2 = np.stack([(j * pw(l1, i) * pw(l2, j - 1)) if j > 0 else 0 * one for i, j in fem2d_p2.MONOMIALS], axis=1)
    dphi = np.stack([d1 @ T.T, d2 @ T.T], axis=2)                         # (M, p, 2): d/dl1, d/dl2
    return np.einsum("mba,mpb->mpa", Ji, dphi)


def _cheb(x, n, dtype):
    """T_j(x) and T_j'(x) = j U_{j-1}(x), j < n, by the recurrences of T and U: arrays x.shape + (n,)."""
    x = x.astype(dtype)
    T = np.empty(x.shape + (n,), dtype=dtype)
    U = np.empty_like(T)
    T[..., 0], U[..., 0] = 1, 1
    if n > 1:
        T[..., 1], U[..., 1] = x, 2 * x
    for j in range(2, n):
        T[..., j] = 2 * x * T[..., j - 1] - T[..., j - 2]
        U[..., j] = 2 * x * U[..., j - 1] - U[..., j - 2]
    dT = np.zeros_like(T)
    for j in range(1, n):
        dT[..., j] = j * U[..., j - 1]
    return T, dT


def _inverse_ld(V):
    """Gauss-Jordan with partial pivoting in longdouble (NumPy's linalg has no extended precision)."""
    n = V.shape[0]
    A = np.concatenate([V.astype(LD), np.eye(n, dtype=LD)], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]] = A[[piv, c]]
        A[c] = A[c] / A[c, c]
        for r in range(n):
            if r != c:
                A[r] = A[r] - A[r, c] * A[c]
    return A[:, n:]


def _spectral_basis_grads(geom, pts):
    """(M, p, d) gradients of the nodal (cardinal) functions of the Chebyshev interpolant in longdouble:
    phi_i = sum_j (V^{-1})_{ji} T_j with V = evaluation(x, n); 2-D: products, node i + n j."""
    d = geom.x.shape[2]
    n = len(geom.w) if d == 1 else geom.discretization.n
    x = geom.xflat[:n, 0]
    Vinv = _inverse_ld(_cheb(x, n, LD)[0])
    if d == 1:
        _, dT = _cheb(pts[:, 0], n, LD)
        return (dT @ Vinv)[:, :, None]
    Tx, dTx = _cheb(pts[:, 0], n, LD)
    Ty, dTy = _cheb(pts[:, 1], n, LD)
    A, dA, B, dB = Tx @ Vinv, dTx @ Vinv, Ty @ Vinv, dTy @ Vinv
    M = pts.shape[0]
    gx = (B[:, :, None] * dA[:, None, :]).reshape(M, -1)                  # index j * n + i
    gy = (dB[:, :, None] * A[:, None, :]).reshape(M, -1)
    return np.stack([gx, gy], axis=2)


def _spectral_twin(geom, z, pts):
    """float64: the coefficients the device receives, float64 sums of c_j T_j'."""
    d = geom.x.shape[2]
    if d == 1:
        c = _spectral1d_coefficients(geom, z[:, None])[:, 0]
        return (_cheb(pts[:, 0], len(c), np.float64)[1] @ c)[:, None]
    n = geom.discretization.n
    C = _spectral2d_coefficients(geom, z[:, None])[:, 0].reshape(n, n)
    Tx, dTx = _cheb(pts[:, 0], n, np.float64)
    Ty, dTy = _cheb(pts[:, 1], n, np.float64)
    return np.stack([np.einsum("mi,ij,mj->m", dTx, C, Ty), np.einsum("mi,ij,mj->m", Tx, C, dTy)], axis=1)


def _kind(geom):
    name = type(geom.discretization).__name__
    return {"TensorFEM": "qk", "FEM2D_P1": "simplex", "FEM2D_P2": "simplex"}.get(name, "spectral")


def host_gradients(geom, z, elem, pts):
    """(oracle gradient (M, d) in longdouble, float64 twin (M, d), S (M,)) in the elements `elem` at `pts` (M, d)."""
    kind = _kind(geom)
    p = geom.x.shape[0]
    if kind == "spectral":
        G = _spectral_basis_grads(geom, pts)
        zl = np.broadcast_to(z.astype(LD), (pts.shape[0], z.shape[0]))
        return np.einsum("mpa,mp->ma", G, zl), _spectral_twin(geom, z, pts), np.abs(G).max(axis=2) @ np.abs(z).astype(LD)
    fn = _qk_basis_grads if kind == "qk" else _simplex_basis_grads
    rows = elem.astype(np.int64)[:, None] * p + np.arange(p)[None, :]
    zl = z[rows]
    G, G64 = fn(geom, elem, pts, LD), fn(geom, elem, pts, np.float64)
    g = np.einsum("mpa,mp->ma", G, zl.astype(LD))
    g64 = np.einsum("mpa,mp->ma", G64, zl)
    return g, g64, (np.abs(G).max(axis=2) * np.abs(zl)).sum(axis=1)


def _ratios(gdev, g, g64, S):
    S = np.maximum(S, LD(1e-300))
    return (float((np.abs(gdev.astype(LD) - g).max(axis=1) / S).max()),
            float((np.abs(g64.astype(LD) - g).max(axis=1) / S).max()))


def _as2d(a):
    return a.reshape(-1, 1) if a.ndim == 1 else a


def _distort(X, a, b):
    """A global (tri)linear distortion of [-1, 1]^d: every element's image is a multilinear (non-affine) cell."""
    Y = X.copy()
    prod = np.prod(X, axis=-1)
    Y[..., 0] += a * prod
    Y[..., 1] += b * prod
    return Y


def _oracle_geom(name, k):
    if name == "fem2d_distorted":
        return m.fem2d(k=k, K=_distort(m.subdivide(m.fem2d(k=k), 3).x, 0.15, -0.1)), 2
    if name == "fem3d_distorted":
        return m.fem3d(k=k, K=_distort(m.subdivide(m.fem3d(k=k), 2).x, 0.15, -0.1)), 3
    geom, d, _ = _repro_geom(name, k)
    return geom, d


def _oracle_points(name, rng, d, M):
    pts = _interior(rng, M, d)
    if name.endswith("distorted"):
        pts = _distort(pts, 0.15, -0.1)              # images of interior points: inside the distorted mesh
    return pts


ORACLE = REPRO + [("fem2d_distorted", 2), ("fem3d_distorted", 1)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. host oracle in extended precision, random z
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k", ORACLE)
def test_gradient_against_extended_precision_oracle(name, k):
    rng = np.random.default_rng(zlib.crc32(f"grad{name}{k}".encode()))
    geom, d = _oracle_geom(name, k)
    z = rng.standard_normal(geom.xflat.shape[0])
    pts = _oracle_points(name, rng, d, 20_000)
    vals, grads, elem = m.interpolate(geom, z, pts[:, 0] if d == 1 else pts, gradient=True, return_element=True)
    assert np.all(elem >= 0) and np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
    g, g64, S = host_gradients(geom, z, elem, pts)
    r_dev, r_twin = _ratios(_as2d(grads), g, g64, S)
    line = (f"interpolate gradient oracle {name} k={k}: device {r_dev / EPS:.2f} eps, float64 twin {r_twin / EPS:.2f} eps "
            f"(of S(q)), allowed {DEVICE_FACTOR * r_twin / EPS:.2f} eps")
    print(line)
    record_observation(line)
    assert r_twin <= TWIN_CAP, line
    assert r_dev <= DEVICE_FACTOR * r_twin, line


# ---------------------------------------------------------------------------------------------------------------------
# 2. polynomial reproduction
# ---------------------------------------------------------------------------------------------------------------------

def _poly_ld(rng, d, k, total):
    """A random polynomial in longdouble with its gradient: degree k per variable, or total degree k."""
    C = rng.standard_normal((k + 1,) * d)
    if total:
        for idx in np.ndindex(*C.shape):
            if sum(idx) > k:
                C[idx] = 0.0

    def f(X, da=None):
        X = np.atleast_2d(X).astype(LD)
        out = np.zeros(X.shape[0], dtype=LD)
        for idx in np.ndindex(*C.shape):
            term = np.full(X.shape[0], LD(C[idx]))
            for a, e in enumerate(idx):
                if a == da:
                    term = term * (e * X[:, a] ** (e - 1) if e > 0 else 0)
                else:
                    term = term * X[:, a] ** e
            out += term
        return out
    return f


@pytest.mark.parametrize("name,k", REPRO)
def test_gradient_reproduces_polynomial_gradients(name, k):
    """z = the nodal values of a polynomial of the element space, rounded once from longdouble: the interpolant's
    gradient differs from the polynomial's by at most (eps / 2) S(q) through that rounding, on top of the device's
    allowance of section 1 (whose margin also covers the rounding of the mesh's own node coordinates)."""
    rng = np.random.default_rng(zlib.crc32(f"gradpoly{name}{k}".encode()))
    geom, d, deg = _repro_geom(name, k)
    f = _poly_ld(rng, d, deg, total=name.startswith("fem2d_P"))
    z = f(geom.xflat).astype(np.float64)
    pts = _interior(rng, 20_000, d)
    vals, grads, elem = m.interpolate(geom, z, pts[:, 0] if d == 1 else pts, gradient=True, return_element=True)
    assert np.all(elem >= 0) and np.all(np.isfinite(vals))                # every interior point is located
    g, g64, S = host_gradients(geom, z, elem, pts)
    exact = np.stack([f(pts, da=a) for a in range(d)], axis=1)
    r_dev, r_twin = _ratios(_as2d(grads), exact, g64, S)                  # both against the analytic gradient
    _, r_twin_oracle = _ratios(_as2d(grads), g, g64, S)
    line = (f"interpolate gradient polynomial {name} k={k}: device {r_dev / EPS:.2f} eps, twin {r_twin_oracle / EPS:.2f} eps")
    print(line)
    record_observation(line)
    assert r_twin_oracle <= TWIN_CAP, line
    assert r_dev <= DEVICE_FACTOR * r_twin_oracle + EPS / 2, line


# ---------------------------------------------------------------------------------------------------------------------
# 3. central differences of device values
# ---------------------------------------------------------------------------------------------------------------------

def test_gradient_agrees_with_central_differences_of_values():
    geom = m.subdivide(m.fem2d_P2(), 4)
    rng = np.random.default_rng(33)
    z = rng.standard_normal(geom.xflat.shape[0])
    pts = _interior(rng, 20_000, 2)
    h = 1e-5
    _, grads, elem = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    keep = elem >= 0
    fd = np.empty_like(grads)
    for a in range(2):
        e = np.zeros(2)
        e[a] = h
        vp, ep = m.interpolate(geom, z, pts + e, return_element=True)
        vm, em = m.interpolate(geom, z, pts - e, return_element=True)
        keep &= (ep == elem) & (em == elem)
        fd[:, a] = (vp - vm) / ((pts[:, a] + h) - (pts[:, a] - h))
    share = float(keep.mean())
    err = float(np.abs(fd[keep] - grads[keep]).max() / np.abs(grads[keep]).max())
    line = f"interpolate gradient vs central differences fem2d_P2 L=4: {share:.4f} of the points kept, rel err {err:.3e}"
    print(line)
    record_observation(line)
    assert share >= 0.9, line
    assert err <= 1e-6, line


# ---------------------------------------------------------------------------------------------------------------------
# 4. the operators the solver uses
# ---------------------------------------------------------------------------------------------------------------------

def _operator_grads(geom, z):
    names = ["dx", "dy", "dz"][:geom.x.shape[2]]
    return np.stack([np.asarray(geom.operators[nm].to_sparse() @ z).reshape(-1) for nm in names], axis=1)


def test_p1_centroid_gradient_is_the_operator_rows():
    """P1: the gradient is constant per element.  The operator rows are float64 results with their own rounding, so
    the device may differ from them by its allowance of section 1 plus the operators' own measured distance from the
    longdouble oracle."""
    geom = m.subdivide(m.fem2d_P1(), 4)
    rng = np.random.default_rng(41)
    z = rng.standard_normal(geom.xflat.shape[0])
    N = geom.x.shape[1]
    cent = geom.x.mean(axis=0)                                            # (N, 2)
    _, grads, elem = m.interpolate(geom, z, cent, gradient=True, return_element=True)
    assert np.array_equal(elem, np.arange(N))
    g, g64, S = host_gradients(geom, z, elem, cent)
    op = _operator_grads(geom, z).reshape(N, 3, 2)
    _, r_twin = _ratios(grads, g, g64, S)
    worst = 0.0
    for i in range(3):
        r_op, _ = _ratios(op[:, i], g, g64, S)
        r_dev = float((np.abs(grads - op[:, i]).max(axis=1) / S.astype(np.float64)).max())
        worst = max(worst, r_dev)
        assert r_dev <= DEVICE_FACTOR * r_twin + r_op, (i, r_dev, r_twin, r_op)
    line = f"interpolate gradient vs operators fem2d_P1 L=4: {worst / EPS:.2f} eps of S(q), twin {r_twin / EPS:.2f} eps"
    print(line)
    record_observation(line)
    assert r_twin <= TWIN_CAP


@pytest.mark.parametrize("name,make", [("fem2d_P2 L=3", lambda: m.subdivide(m.fem2d_P2(), 3)),
                                       ("fem3d k=2 L=2", lambda: m.subdivide(m.fem3d(k=2), 2))])
def test_node_gradients_follow_the_operator_layout(name, make):
    geom = make()
    p, N, d = geom.x.shape
    rng = np.random.default_rng(43)
    a = rng.standard_normal((d, d))
    X = geom.xflat
    z = np.sin(X @ a[0]) + 0.5 * (X @ a[1]) ** 2                          # smooth: the pull moves the gradient little
    cent = geom.x.mean(axis=0)                                            # (N, d)
    own = np.repeat(np.arange(N), p)                                      # row e * p + i belongs to element e
    pts = X + 1e-3 * (cent[own] - X)
    _, grads, elem = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(elem, own)
    op = _operator_grads(geom, z)
    err = float(np.abs(grads - op).max() / np.abs(op).max())
    line = f"interpolate gradient vs operator rows at pulled nodes {name}: rel err {err:.3e}"
    print(line)
    record_observation(line)
    assert err <= 1e-2, line


# ---------------------------------------------------------------------------------------------------------------------
# 5. semantics
# ---------------------------------------------------------------------------------------------------------------------

SEMANTIC = [("fem1d", 3), ("fem2d", 2), ("fem3d", 2), ("fem2d_P1", 1), ("fem2d_P2", 2), ("spectral1d", 16),
            ("spectral2d", 7)]


@pytest.mark.parametrize("name,k", SEMANTIC)
def test_values_columns_and_repeats_are_bitwise(name, k):
    geom, d, _ = _repro_geom(name, k)
    rng = np.random.default_rng(zlib.crc32(f"sem{name}".encode()))
    Z = rng.standard_normal((geom.xflat.shape[0], 3))
    pts = np.concatenate([_interior(rng, 5_000, d), geom.xflat[::3]])
    t = pts[:, 0] if d == 1 else pts
    v0, e0 = m.interpolate(geom, Z, t, return_element=True)
    v1, g1, e1 = m.interpolate(geom, Z, t, gradient=True, return_element=True)
    assert np.array_equal(v0, v1) and np.array_equal(e0, e1)
    assert g1.shape == (v1.shape + (d,) if d > 1 else v1.shape)
    v2, g2 = m.interpolate(geom, Z, t, gradient=True)
    assert np.array_equal(v1, v2) and np.array_equal(g1, g2)              # two identical calls
    for j in range(3):
        vj, gj = m.interpolate(geom, Z[:, j], t, gradient=True)
        assert np.array_equal(vj, v1[:, j]) and np.array_equal(gj, g1[:, j])
        assert np.array_equal(vj, m.interpolate(geom, Z[:, j], t))
    # one point: scalars / short vectors
    one = m.interpolate(geom, Z[:, 0], t[7], gradient=True)
    assert isinstance(one[0], float) and np.array_equal(np.asarray(one[1]), g1[7, 0])
    assert isinstance(one[1], float) if d == 1 else one[1].shape == (d,)


@pytest.mark.parametrize("name,k", [("fem2d", 2), ("fem3d", 1), ("fem2d_P1", 1), ("fem2d_P2", 2)])
def test_unlocated_points_have_nan_gradients(name, k):
    geom, d, _ = _repro_geom(name, k)
    z = np.random.default_rng(2).standard_normal((geom.xflat.shape[0], 2))
    bad = np.zeros((6, d))
    bad[0, 0], bad[1, d - 1], bad[2, :] = 1.5, -1.0 - 1e-6, 3.0
    bad[3, 0], bad[4, d - 1], bad[5, 0] = np.nan, np.inf, -np.inf
    pts = np.concatenate([bad, np.zeros((1, d)) + 0.123])
    v, g, e = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.all(np.isnan(v[:6])) and np.all(np.isnan(g[:6])) and np.all(e[:6] == -1)
    assert np.all(np.isfinite(g[6])) and e[6] >= 0
    assert np.all(np.isnan(m.interpolate(geom, z[:, 0], np.full(d, 2.0), gradient=True)[1]))


def test_fem1d_clamp_and_one_sided_end_derivatives():
    geom = m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 3), k=3), 2)
    rng = np.random.default_rng(6)
    z = rng.standard_normal(geom.xflat.shape[0])
    pts = np.array([-3.0, -1.0 - 1e-15, -np.inf, np.inf, 1.0 + 1e-15, 2.5, -1.0, 1.0, np.nan])
    v, g, e = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(g[:6], np.zeros(6)) and not np.any(np.signbit(g[:6]))
    assert np.isnan(g[8]) and np.isnan(v[8])
    N = geom.x.shape[1]
    assert e[6] == 0 and e[7] == N - 1
    ends = np.array([[-1.0], [1.0]])
    gh, g64, S = host_gradients(geom, z, np.array([0, N - 1]), ends)
    r_dev, r_twin = _ratios(g[6:8].reshape(2, 1), gh, g64, S)
    # also against one-sided difference quotients of the end elements' interpolants (formula-free, coarse)
    hh = 1e-6
    vv = m.interpolate(geom, z, np.array([-1.0, -1.0 + hh, 1.0 - hh, 1.0]))
    fd = np.array([(vv[1] - vv[0]) / hh, (vv[3] - vv[2]) / hh])
    line = (f"interpolate gradient fem1d end points: device {r_dev / EPS:.2f} eps, twin {r_twin / EPS:.2f} eps; "
            f"vs one-sided quotient {np.abs(fd - g[6:8]).max():.2e}")
    print(line)
    record_observation(line)
    assert r_dev <= DEVICE_FACTOR * max(r_twin, EPS), line
    assert np.abs(fd - g[6:8]).max() <= 1e-3 * max(1.0, np.abs(g[6:8]).max())
    # an interior shared node takes the element the value takes (its left end, xi = -1)
    node = geom.x[0, 1, 0]
    _, gn, en = m.interpolate(geom, z, np.array([node]), gradient=True, return_element=True)
    ghn, g64n, Sn = host_gradients(geom, z, en, np.array([[node]]))
    assert en[0] == 1 and _ratios(gn.reshape(1, 1), ghn, g64n, Sn)[0] <= DEVICE_FACTOR * max(r_twin, EPS)


@pytest.mark.parametrize("n", [4, 16])
def test_spectral_gradients_at_the_end_points(n):
    rng = np.random.default_rng(n)
    g1 = m.spectral1d(n=n)
    z1 = rng.standard_normal(n)
    t = np.array([-1.0, 1.0, -1.0 + 1e-9, 0.3, np.nan, np.inf])
    v, g = m.interpolate(g1, z1, t, gradient=True)
    assert np.all(np.isfinite(g[:4])) and np.all(np.isnan(g[4:])) and np.all(np.isnan(v[4:]))
    gh, g64, S = host_gradients(g1, z1, None, t[:4, None])
    r1, t1 = _ratios(g[:4, None], gh, g64, S)
    g2 = m.spectral2d(n=n)
    z2 = rng.standard_normal(n * n)
    P = np.array([[-1.0, -1.0], [1.0, 1.0], [1.0, -1.0], [-1.0, 0.4], [0.2, 1.0], [0.1, -0.7]])
    _, gg = m.interpolate(g2, z2, P, gradient=True)
    assert np.all(np.isfinite(gg))
    gh2, g642, S2 = host_gradients(g2, z2, None, P)
    r2, t2 = _ratios(gg, gh2, g642, S2)
    line = (f"interpolate gradient spectral n={n} at +-1: 1-D device {r1 / EPS:.2f} eps (twin {t1 / EPS:.2f}), "
            f"2-D device {r2 / EPS:.2f} eps (twin {t2 / EPS:.2f})")
    print(line)
    record_observation(line)
    assert max(t1, t2) <= TWIN_CAP
    assert r1 <= DEVICE_FACTOR * t1 and r2 <= DEVICE_FACTOR * t2, line
    assert np.all(np.isnan(m.interpolate(g2, z2, np.array([[np.nan, 0.0], [0.0, np.inf]]), gradient=True)[1]))


@pytest.mark.parametrize("name,make,L,shift,deg", [c for c in SHIFTED if "Q1" in c[0]])
def test_translated_q1_meshes_still_locate_every_point(name, make, L, shift, deg):
    geom = m.subdivide(make(), L)
    d = geom.x.shape[2]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    a = rng.standard_normal(3)
    z = a[0] + a[1] * (geom.xflat[:, 0] - shift) + a[2] * (geom.xflat[:, d - 1] - shift)
    pts = shift + _interior(rng, 200_000, d, margin=0.0)
    vals, grads, elem = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    missing = int(np.count_nonzero(elem < 0))
    exact = np.zeros(d)
    exact[0] += a[1]
    exact[d - 1] += a[2]
    err = float(np.abs(grads - exact).max()) if missing == 0 else float("nan")
    line = f"interpolate gradient translated {name} L={L}: {missing} points not found, max abs err {err:.3e}"
    print(line)
    record_observation(line)
    assert missing == 0 and np.all(np.isfinite(grads))
    assert np.array_equal(vals, m.interpolate(geom, z, pts))
    # an affine function: the nodal values carry eps * shift-sized rounding of the coordinates, over elements of size h
    assert err <= 64 * EPS * shift * 2 ** L * max(1.0, np.abs(a).max()), line


def test_fine_q1_mesh_still_locates_every_point():
    geom = m.subdivide(m.fem2d(k=1), 11)                                  # 1024 x 1024 elements
    rng = np.random.default_rng(1024)
    a = rng.standard_normal(3)
    z = a[0] + a[1] * geom.xflat[:, 0] + a[2] * geom.xflat[:, 1]
    pts = _interior(rng, 2_000_000, 2, margin=0.0)
    _, grads, elem = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    missing = int(np.count_nonzero(elem < 0))
    err = float(np.abs(grads - a[1:]).max()) if missing == 0 else float("nan")
    line = f"interpolate gradient fem2d Q1 L=11, 2M points: {missing} not found, max abs err {err:.3e}"
    print(line)
    record_observation(line)
    assert missing == 0, line
    assert err <= 64 * EPS * 2 ** 11 * max(1.0, np.abs(a).max()), line


# ---------------------------------------------------------------------------------------------------------------------
# 6. a real solve: the plastic zone of elastoplastic torsion
# ---------------------------------------------------------------------------------------------------------------------

def test_elastoplastic_torsion_plastic_zone():
    """P1: the gradient is constant per element, so the nodal constraint |grad u| <= smax holds at every point.  The
    default load f = 4 yields: the unconstrained torsion function of the square [-1, 1]^2 has max |grad u| = 0.675 f."""
    smax = 1.0
    geom = m.subdivide(m.fem2d_P1(), 4)
    sol = m.mgb_solve(m.Zoo.elastoplastic_torsion(m.amg(geom), smax=smax))
    rng = np.random.default_rng(66)
    pts = _interior(rng, 2_000, 2)
    _, grads, elem = m.interpolate(geom, sol.z[:, 0], pts, gradient=True, return_element=True)
    assert np.all(elem >= 0)
    norm = np.sqrt((grads ** 2).sum(axis=1))
    plastic = norm > 0.99 * smax
    line = (f"interpolate gradient elastoplastic torsion fem2d_P1 L=4: max |grad u| {norm.max():.12f}, plastic share "
            f"{plastic.mean():.3f}")
    print(line)
    record_observation(line)
    assert norm.max() <= smax * (1 + 1e-9), line
    assert 0 < plastic.sum() < plastic.size, line
