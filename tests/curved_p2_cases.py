"""Curved fem2d_P2 for tests/test_curved_p2.py and tests/test_gpu_curved_p2.py: the two meshes, manufactured points
and the host references (an np.longdouble oracle and a float64 NumPy twin of the device's Newton iteration).

Mesh A: the 32 elements of `subdivide(fem2d_P2(), 3)` under the smooth non-polynomial map `_curve` of
tests/test_gpu_locator.py, applied to every node: really curved edges, bubbles off the centroid.
Mesh B: two elements whose shared edge bulges out of the box of element 0's nodes (its edge node lies at y = -0.1, the
edge's quadratic dips to about y = -0.1125): what the padded element boxes are for.

A manufactured point is made, not found: pick an element and a barycentric pair, form the point by the forward map
sum_j phi_j(l1, l2) x_j in np.longdouble and round it to float64.  No inversion is needed to know where it lies.
"""
import numpy as np

import mgb_amd as m
from mgb_amd import fem2d_p2

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
# csrc/interp_device.hpp
NEWTON_MAXIT, NEWTON_STEP_TOL, ROUND_FACTOR, ACCEPT_TOL = 32, 1e-13, 64.0, 1e-11


def mesh_a(bubble, curved=True):
    X0 = m.subdivide(m.fem2d_P2(bubble=bubble), 3).x
    X = X0.copy()
    X[..., 0] += 0.08 * np.sin(np.pi * X0[..., 1])
    X[..., 1] += 0.06 * np.sin(np.pi * X0[..., 0]) * X0[..., 1]
    return m.fem2d_P2(bubble=bubble, K=X, curved=curved)


def mesh_b(bubble, curved=True):
    corners = np.array([[(0.0, 0.0), (1.0, -0.1), (0.5, 1.0)], [(1.0, -0.1), (0.0, 0.0), (0.5, -1.0)]])
    K = np.zeros((7 if bubble else 6, 2, 2))
    for e in range(2):
        c = corners[e]
        K[0, e], K[2, e], K[4, e] = c[0], c[1], c[2]
        K[1, e] = (0.5, -0.1)                               # the shared edge's node, in both elements
        K[3, e] = 0.5 * (c[1] + c[2])
        K[5, e] = 0.5 * (c[2] + c[0])
        if bubble:
            K[6, e] = (4.0 / 9.0) * (K[1, e] + K[3, e] + K[5, e]) - (1.0 / 9.0) * (c[0] + c[1] + c[2])
    return m.fem2d_P2(bubble=bubble, K=K, curved=curved)


MESHES = {"A": mesh_a, "B": mesh_b}


def basis(p, l, dtype):
    """phi (M, p) and dphi/dl (M, p, 2) at the barycentric pairs l (M, 2), from the 10-monomial table in `dtype`."""
    T = fem2d_p2.basis_coefficient_table(p == 7).astype(dtype)
    l1, l2 = l[:, 0].astype(dtype), l[:, 1].astype(dtype)
    one = np.ones_like(l1)
    pw = lambda v, e: one if e == 0 else v ** e
    mono = np.stack([pw(l1, i) * pw(l2, j) for i, j in fem2d_p2.MONOMIALS], axis=1)
    d1 = np.stack([(i * pw(l1, i - 1) * pw(l2, j)) if i > 0 else 0 * one for i, j in fem2d_p2.MONOMIALS], axis=1)
    d2 = np.stack([(j * pw(l1, i) * pw(l2, j - 1)) if j > 0 else 0 * one for i, j in fem2d_p2.MONOMIALS], axis=1)
    return mono @ T.T, np.stack([d1 @ T.T, d2 @ T.T], axis=2)


def element_nodes(geom, elem, dtype):
    return geom.x.astype(dtype)[:, elem, :].transpose(1, 0, 2)                 # (M, p, 2)


def forward(geom, elem, l):
    """The points made in the elements `elem` at the pairs `l`: the forward map in longdouble, rounded to float64."""
    phi, _ = basis(geom.x.shape[0], l, LD)
    return np.einsum("mp,mpa->ma", phi, element_nodes(geom, elem, LD)).astype(np.float64)


def manufactured(geom, rng, M, lmin=0.02):
    """(elements (M,), pairs (M, 2), points (M, 2)) with every barycentric coordinate >= lmin."""
    elem = rng.integers(0, geom.x.shape[1], size=M)
    lam = lmin + (1.0 - 3.0 * lmin) * rng.dirichlet([1.0, 1.0, 1.0], size=M)
    l = np.ascontiguousarray(lam[:, :2])
    return elem, l, forward(geom, elem, l)


def inv2(J):
    """Inverse of (M, 2, 2) matrices by cofactors in J's dtype, and |J^{-1}|_inf."""
    det = J[:, 0, 0] * J[:, 1, 1] - J[:, 0, 1] * J[:, 1, 0]
    Ji = np.empty_like(J)
    Ji[:, 0, 0], Ji[:, 0, 1] = J[:, 1, 1] / det, -J[:, 0, 1] / det
    Ji[:, 1, 0], Ji[:, 1, 1] = -J[:, 1, 0] / det, J[:, 0, 0] / det
    return Ji, np.abs(Ji).sum(axis=2).max(axis=1)


def affine_start(Xe, P):
    """The barycentric pair of P in the straight triangle of the corner slots 0, 2, 4 (what the device starts from)."""
    o = Xe[:, 4]
    a, b, r = Xe[:, 0] - o, Xe[:, 2] - o, P - o
    det = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    return np.stack([(r[:, 0] * b[:, 1] - r[:, 1] * b[:, 0]) / det, (a[:, 0] * r[:, 1] - a[:, 1] * r[:, 0]) / det], axis=1)


def newton(geom, elem, pts, dtype, start=None):
    """The pairs (M, 2) of pts in the elements elem, the iterations each point took, whether it was accepted and the
    stopping tolerance it met.
    longdouble: 40 full Newton steps from `start` (the manufactured pairs).  float64: the device's rule restated: start
    from the affine pair of the corners, stop once max|dl| <= max(1e-13, 64 eps max|x| |J^{-1}|_inf), 32 steps at
    most, accept iff l1, l2, 1 - l1 - l2 >= -max(1e-11, that tolerance)."""
    p = geom.x.shape[0]
    Xe = element_nodes(geom, elem, dtype)
    P = pts.astype(dtype)
    exact = dtype is LD
    l = start.astype(dtype) if exact else affine_start(Xe, P)
    M = P.shape[0]
    done = np.zeros(M, dtype=bool)
    its = np.zeros(M, dtype=np.int64)
    tol = np.full(M, NEWTON_STEP_TOL)
    xs = np.maximum(np.abs(Xe).max(axis=(1, 2)), np.abs(P).max(axis=1))
    for _ in range(40 if exact else NEWTON_MAXIT):
        phi, dphi = basis(p, l, dtype)
        F = np.einsum("mp,mpa->ma", phi, Xe) - P
        J = np.einsum("mpb,mpa->mab", dphi, Xe)
        Ji, ninv = inv2(J)
        dl = np.einsum("mab,mb->ma", Ji, F)
        l = np.where(done[:, None], l, l - dl)
        if not exact:
            its += ~done
            t = np.maximum(NEWTON_STEP_TOL, ROUND_FACTOR * EPS * xs * ninv).astype(np.float64)
            tol = np.where(done, tol, t)
            done |= np.abs(dl).max(axis=1) <= t
            if done.all():
                break
    if exact:
        return l, its, np.ones(M, dtype=bool), tol
    acc = np.maximum(ACCEPT_TOL, tol)
    ok = done & (l[:, 0] >= -acc) & (l[:, 1] >= -acc) & (1.0 - l[:, 0] - l[:, 1] >= -acc)
    return l, its, ok, tol


def host_reference(geom, z, elem, pts, made):
    """Values and gradients of the element-space function z in the elements elem at pts, on the host:
    (oracle values (M,), twin values, value scale; oracle gradients (M, 2), twin gradients, S), the oracle in longdouble
    with Newton from the manufactured pairs `made`, the twin in float64 with the device's stopping rule.

    S(q) = sum_i |grad_x phi_i(q)|_inf |z_i| is the rounding scale of the gradient sum; the value's scale is
    sum_i |phi_i(q)| |z_i| + max|x| S(q): the rounding of the sum plus the rounding of the point."""
    p = geom.x.shape[0]
    zl = z[elem.astype(np.int64)[:, None] * p + np.arange(p)[None, :]]
    res = {}
    for dtype in (LD, np.float64):
        l = newton(geom, elem, pts, dtype, start=made)[0]
        phi, dphi = basis(p, l, dtype)
        Xe = element_nodes(geom, elem, dtype)
        Ji, _ = inv2(np.einsum("mpb,mpa->mab", dphi, Xe))
        G = np.einsum("mba,mpb->mpa", Ji, dphi)                                   # grad_x phi_i
        Z = zl.astype(dtype)
        res[dtype] = ((phi * Z).sum(axis=1), np.einsum("mpa,mp->ma", G, Z), phi, G)
    v, g, phi, G = res[LD]
    S = (np.abs(G).max(axis=2) * np.abs(zl)).sum(axis=1)
    Sv = (np.abs(phi) * np.abs(zl)).sum(axis=1) + LD(np.abs(geom.xflat).max()) * S
    return v, res[np.float64][0], Sv, g, res[np.float64][1], S


def ratios(dev, ref, twin, scale):
    """(largest device error, largest twin error) against the oracle `ref`, in units of `scale` per point."""
    scale = np.maximum(scale, LD(1e-300))
    red = (lambda a: a.max(axis=1)) if np.ndim(ref) == 2 else (lambda a: a)
    return (float((red(np.abs(np.asarray(dev).astype(LD) - ref)) / scale).max()),
            float((red(np.abs(np.asarray(twin).astype(LD) - ref)) / scale).max()))
