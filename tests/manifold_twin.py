"""A plain NumPy restatement of the lattice, the triangle enumeration and the cut of `isocontour()` / `tessellate()` for
2-D elements in `e` = 2 or 3 coordinates: the yardstick of tests/test_manifold_post.py and
tests/test_gpu_manifold_post.py.  For `e = 2` it is tests/contour_twin.py operation for operation (the tests assert the
two equal bitwise); the ambient dimension only adds coordinates, each formed on its own:

1. lattice: every element sampled with its own basis at `refine + 1` equispaced points per axis of [-1, 1] (Q_k, axis 0
   fastest) or on the barycentric lattice (P1 / P2); every field and every one of the `e` coordinates is a sum over the
   element's nodes in ascending local index, one multiplication and one addition per node;
2. triangles: per lattice square (i fastest) [(i,j), (i+1,j), (i+1,j+1)] and [(i,j), (i,j+1), (i+1,j+1)]; P1 / P2 as in
   tests/contour_twin.py.  `tessellate_twin` emits them all, triangle i of element n at n * ntri + i;
3. cutting: value >= c is above; an edge (a, b) of lattice indices a < b is crossed at t = (c - v_a) / (v_b - v_a),
   x[c] = x_a[c] + t (x_b[c] - x_a[c]) per coordinate; cut edges in ascending (a, b);
4. order: element, cell, triangle of the cell, level index.

Per emitted vertex the twin reports `dv`, `dx`, `dc` and per call `margin` as `isocontour_twin` does, and in addition
where the vertex came from: the tessellation triangle (`tri`) and the two corners of it (`qa`, `qb`) its edge joins.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from mgb_amd.tensorfem import TensorFEM, _tf_nodes

from contour_twin import _basis_and_simplices, _lagrange
from contour_twin import default_refine  # noqa: F401  (re-exported)


@dataclass
class TwinSurfaceContour:
    points: np.ndarray        # (S, 2, e)
    level: np.ndarray
    element: np.ndarray
    carried: Optional[np.ndarray]
    nlevels: int
    dv: np.ndarray            # (S, 2): |v_b - v_a| of the edge each vertex lies on
    dx: np.ndarray            # (S, 2): max over the coordinates of |x_b - x_a|
    dc: Optional[np.ndarray]  # (S, 2, ncarry)
    margin: float             # min over lattice points and levels of |value - level| (inf if there is none)
    tri: np.ndarray           # (S,): element * ntri + triangle of the element
    qa: np.ndarray            # (S, 2): corner (0..2) of that triangle at the lower end of the vertex's edge
    qb: np.ndarray            # (S, 2): ... at the upper end

    def measure(self) -> np.ndarray:
        P = self.points
        if P.shape[2] == 2:
            m = np.hypot(P[:, 1, 0] - P[:, 0, 0], P[:, 1, 1] - P[:, 0, 1])
        else:
            m = np.sqrt(np.sum((P[:, 1] - P[:, 0]) ** 2, axis=1))
        return np.bincount(self.level, weights=m, minlength=self.nlevels).astype(np.float64)


@dataclass
class TwinTessellation:
    points: np.ndarray        # (T, 3, e)
    element: np.ndarray       # (T,)
    values: Optional[np.ndarray]

    def measure(self) -> float:
        P = self.points
        a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        if P.shape[2] == 3:
            return float(np.sum(0.5 * np.linalg.norm(np.cross(a, b), axis=1)))
        return float(np.sum(0.5 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])))


def basis_and_triangles(geom, r):
    """(phi (npts, p): every local basis function at every lattice point, triangles (ntri, 3) of lattice indices)."""
    disc = geom.discretization
    if not isinstance(disc, TensorFEM):
        return _basis_and_simplices(geom, r)
    assert disc.d == 2
    p = geom.x.shape[0]
    k = disc.k
    nodes = _tf_nodes(k)
    S, n1 = k + 1, r + 1
    B = np.stack([_lagrange(nodes, -1.0 + (2.0 * i) / r) for i in range(n1)])
    phi = np.empty((n1 * n1, p))
    for pt in range(n1 * n1):
        i, j = pt % n1, pt // n1
        for node in range(p):
            phi[pt, node] = B[i, node % S] * B[j, node // S]
    simp = []
    for j in range(r):
        for i in range(r):
            b = j * n1 + i
            simp += [(b, b + 1, b + n1 + 1), (b, b + n1, b + n1 + 1)]
    return phi, np.array(simp, dtype=np.int64)


def lattice(geom, fields, refine=None):
    """(X (N, npts, e), F (N, npts, nfield) or None, triangles): steps 1 and 2."""
    p, N, e = geom.x.shape
    r = default_refine(geom) if refine is None else refine
    phi, simp = basis_and_triangles(geom, r)
    npts = phi.shape[0]
    Xn = np.asarray(geom.xflat, dtype=np.float64).reshape(N, p, e)
    Fn = None if fields is None else np.asarray(fields, dtype=np.float64).reshape(N, p, -1)
    X = np.zeros((N, npts, e))
    F = None if Fn is None else np.zeros((N, npts, Fn.shape[2]))
    with np.errstate(invalid="ignore", over="ignore"):
        for node in range(p):                       # ascending local node: one product and one addition per node
            X = X + phi[None, :, node, None] * Xn[:, None, node, :]
            if F is not None:
                F = F + phi[None, :, node, None] * Fn[:, None, node, :]
    return X, F, simp


def tessellate_twin(geom, fields=None, refine=None) -> TwinTessellation:
    X, F, simp = lattice(geom, fields, refine)
    N, ntri = X.shape[0], simp.shape[0]
    pts = X[:, simp].reshape(N * ntri, 3, X.shape[2])
    vals = None if F is None else F[:, simp].reshape(N * ntri, 3, F.shape[2])
    return TwinTessellation(pts, np.repeat(np.arange(N, dtype=np.int32), ntri), vals)


def isocontour_twin_e(geom, z, levels, refine=None, carry=None) -> TwinSurfaceContour:
    lev = np.asarray(levels, dtype=np.float64).reshape(-1)
    nlev = lev.shape[0]
    p, N, e = geom.x.shape
    Z = np.asarray(z, dtype=np.float64).reshape(p * N, 1)
    F = Z if carry is None else np.concatenate([Z, np.asarray(carry, dtype=np.float64).reshape(p * N, -1)], axis=1)
    X, Fl, simp = lattice(geom, F, refine)
    V, Cv = Fl[..., 0], (Fl[..., 1:] if carry is not None else None)
    nc = 0 if Cv is None else Cv.shape[2]
    ntri = simp.shape[0]
    fin = np.isfinite(V)
    margin = float(np.abs(V[fin][:, None] - lev[None, :]).min()) if nlev and fin.any() else float("inf")
    edges = [(0, 1), (0, 2), (1, 2)]                                     # ascending (a, b): the vertices ascend
    val = V[:, simp]                                                     # (N, ntri, 3)
    with np.errstate(invalid="ignore"):
        above = val[:, :, None, :] >= lev[None, None, :, None]           # (N, ntri, nlev, 3)
    ok = np.isfinite(val).all(axis=2)[:, :, None]
    cross = ok & above.any(axis=3) & ~above.all(axis=3)
    ei, si, li = np.nonzero(cross)                                       # C order: element, triangle, level
    S = ei.size
    empty = TwinSurfaceContour(np.empty((0, 2, e)), np.empty(0, dtype=np.int32), np.empty(0, dtype=np.int32),
                               np.empty((0, 2, nc)) if nc else None, nlev, np.empty((0, 2)), np.empty((0, 2)),
                               np.empty((0, 2, nc)) if nc else None, margin, np.empty(0, dtype=np.int64),
                               np.empty((0, 2), dtype=np.int64), np.empty((0, 2), dtype=np.int64))
    if S == 0:
        return empty
    ab = above[ei, si, li]                                               # (S, 3)
    cut = np.stack([ab[:, a] != ab[:, b] for a, b in edges], axis=1)
    assert np.all(cut.sum(axis=1) == 2)
    order = np.argsort(~cut, axis=1, kind="stable")[:, :2]               # the two cut edges, in ascending (a, b)
    qa = np.array([a for a, _ in edges])[order]                          # (S, 2)
    qb = np.array([b for _, b in edges])[order]
    la, lb = simp[si[:, None], qa], simp[si[:, None], qb]
    E = ei[:, None]
    c = lev[li][:, None]
    va, vb = V[E, la], V[E, lb]
    t = (c - va) / (vb - va)
    xa, xb = X[E, la], X[E, lb]
    pts = xa + t[..., None] * (xb - xa)
    car = dcs = None
    if nc:
        ca, cb = Cv[E, la], Cv[E, lb]
        car = ca + t[..., None] * (cb - ca)
        dcs = np.abs(cb - ca)
    return TwinSurfaceContour(pts, li.astype(np.int32), ei.astype(np.int32), car, nlev, np.abs(vb - va),
                              np.abs(xb - xa).max(axis=2), dcs, margin, ei * ntri + si, qa, qb)


def cubed_sphere(m, k=1):
    """The mesh tensor `K` of `fem2d(k=k, K=K, ambient=3)`: each face of the cube [-1, 1]^3 cut into m x m quads whose
    nodes (the 4 corners for k = 1, all (k + 1)^2 tensor nodes otherwise, axis 0 fastest) are projected onto the unit
    sphere.  6 m^2 elements."""
    nodes = np.array([-1.0, 1.0]) if k == 1 else _tf_nodes(k)
    s = len(nodes)
    els = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = [ax for ax in range(3) if ax != axis]
            for jj in range(m):
                for ii in range(m):
                    u0, v0, h = -1.0 + 2.0 * ii / m, -1.0 + 2.0 * jj / m, 2.0 / m
                    P = np.empty((s * s, 3))
                    for j in range(s):
                        for i in range(s):
                            q = np.empty(3)
                            q[axis] = sign
                            q[a] = u0 + 0.5 * (nodes[i] + 1.0) * h
                            q[b] = v0 + 0.5 * (nodes[j] + 1.0) * h
                            P[j * s + i] = q / np.sqrt(np.sum(q * q))
                    els.append(P)
    return np.stack(els, axis=1)
