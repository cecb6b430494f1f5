"""The soups of tests/test_weld.py (twins alone, CPU) and tests/test_gpu_weld.py (the device against the twin).

Synthetic soups have exact answers.  Real soups are level sets and tessellations: `real_soup(name, device)` cuts them with
the NumPy twins of `isocontour()` / `tessellate()` on the CPU and with the package itself on the GPU.  Every soup stays at
M <= 6000 corners, so that the twin's M^2 pair predicate is cheap.
"""
import numpy as np

import mgb_amd as m
from mgb_amd.weld import IndexedMesh


def as_mesh(t, level=None) -> IndexedMesh:
    """The twin's result as an `IndexedMesh`, for its host-side queries."""
    return IndexedMesh(t.vertices, t.cells, t.first_corner, t.component, t.ncomponents, t.normals, t.vertex_data, level,
                       None, t.tol, (0, 0))


# ---------------------------------------------------------------------------------------------------------------------
# synthetic soups
# ---------------------------------------------------------------------------------------------------------------------

def tetrahedron():
    """The tetrahedron on four alternate corners of the cube [-1, 1]^3 as 4 triangles wound outwards; the outward normal
    at vertex p is p / sqrt(3)."""
    p = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
    faces = [(0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)]
    tri = np.array([[p[a], p[b], p[c]] for a, b, c in faces])
    centre = tri.mean(axis=1)
    nrm = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    flip = np.sum(nrm * centre, axis=1) < 0
    tri[flip] = tri[flip][:, [0, 2, 1]]
    return tri


def two_triangles():
    return np.array([[[0.0, 0.0], [1.0, 0.0], [1.0, 1.0]], [[0.0, 0.0], [1.0, 1.0], [0.0, 1.0]]])


def square_polyline():
    c = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    return np.stack([c, np.roll(c, -1, axis=0)], axis=1)


def polyline(S, e=2):
    """An open zigzag of S segments (S + 1 vertices), corners shared bit for bit."""
    i = np.arange(S + 1, dtype=np.float64)
    p = np.stack([i * 0.37, np.sin(i * 0.9) + 0.01 * i, np.cos(i * 0.5)][:e], axis=1)
    return np.stack([p[:-1], p[1:]], axis=1)


def triangle_strip(S):
    """A strip of S triangles in R^3 (S + 2 vertices), corners shared bit for bit."""
    i = np.arange(S + 2, dtype=np.float64)
    p = np.stack([0.5 * i, (np.arange(S + 2) % 2).astype(np.float64), 0.1 * np.sin(i)], axis=1)
    return np.stack([p[:-2], p[1:-1], p[2:]], axis=1)


def straddling_pairs(npairs=500, seed=7):
    """`(soup (2 npairs, 2, 3), tol)`: pairs of points 0.5 tol apart in the max-norm at seeded pseudo-random places in the
    unit cube, each point the first end of its own segment whose other end is far away.  Two far ends are pinned so that
    the largest extent is exactly 2 and `tol = 2 / 512` is the grid's cell side.  All points sit on a jittered lattice of
    pitch 16 tol with a jitter below 8 tol, so different clusters stay more than 4 tol apart (the tests assert that on the
    input with `cluster_separation`)."""
    rng = np.random.default_rng(seed)
    tol = 2.0 / 512
    n = 2 * npairs                       # the near clusters, then the far ends
    side = int(np.ceil(n ** (1.0 / 3.0)))
    assert side * 16 * tol <= 0.7
    slots = rng.permutation(side ** 3)[:n]
    base = np.stack([slots % side, (slots // side) % side, slots // side ** 2], axis=1) * (16 * tol)
    base = base + rng.uniform(0.0, 7 * tol, size=(n, 3))
    near, far = base[:npairs], base[npairs:] + np.array([1.0, 0.0, 0.0])
    delta = 0.5 * tol * rng.choice([-1.0, 1.0], size=(npairs, 3)) * rng.uniform(0.2, 1.0, size=(npairs, 3))
    delta[np.arange(npairs), rng.integers(0, 3, npairs)] = 0.5 * tol      # one axis at 0.5 tol
    soup = np.concatenate([np.stack([near, far], axis=1),
                           np.stack([near + delta, far + np.array([0.0, 0.0, 0.75])], axis=1)])
    soup[0, 1] = [-0.25, 0.0, 0.0]        # pin the box: x runs from -0.25 to 1.75
    soup[1, 1] = [1.75, 1.0, 1.0]
    return soup, tol


def cluster_separation(soup, npairs, tol):
    """The smallest max-norm distance between points of different clusters (pair k is corners (k, 0) and (k + npairs, 0);
    every far end is a cluster of its own)."""
    P = np.concatenate([soup[:, 0], soup[:, 1]])
    cid = np.concatenate([np.arange(npairs), np.arange(npairs), npairs + np.arange(2 * npairs)])
    D = np.abs(P[:, None, :] - P[None, :, :]).max(-1)
    D[cid[:, None] == cid[None, :]] = np.inf
    return float(D.min())


def chain(spacing_in_tol, n=64):
    """`(soup (n, 2, 3), tol)`: n collinear corners `spacing_in_tol * tol` apart, each the first end of its own segment
    whose other end is far from everything."""
    tol = 2.0 ** -9
    i = np.arange(n, dtype=np.float64)
    a = np.stack([i * (spacing_in_tol * tol), np.zeros(n), np.zeros(n)], axis=1)
    b = np.stack([i * 0.03, 1.0 + 0.02 * i, np.ones(n)], axis=1)
    return np.stack([a, b], axis=1), tol


def spirals(nspirals, nseg=4096, seed=11):
    """`(soup, vertex_of_corner)`: polyline spirals of `nseg` segments each (interleaved when there are two), the segments
    in a seeded random order and each in a random orientation.  The corners are bitwise copies of the spiral points, so
    `tol = 0` welds them; `vertex_of_corner` numbers the points by their lowest corner (computed from the construction)."""
    rng = np.random.default_rng(seed)
    pts, segs = [], []
    for s in range(nspirals):
        t = np.linspace(0.0, 1.0, nseg + 1)
        ang = 2 * np.pi * 8 * t + np.pi * s
        r = 0.2 + 0.8 * t
        base = len(pts) * (nseg + 1)
        pts.append(np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1))
        segs.append(np.stack([np.arange(nseg), np.arange(nseg) + 1], axis=1) + base)
    pts, segs = np.concatenate(pts), np.concatenate(segs)
    segs = segs[rng.permutation(segs.shape[0])]
    flip = rng.random(segs.shape[0]) < 0.5
    segs[flip] = segs[flip][:, ::-1]
    assert np.unique(pts, axis=0).shape[0] == pts.shape[0]
    flat = segs.reshape(-1)
    lowest = np.full(pts.shape[0], flat.size, dtype=np.int64)
    np.minimum.at(lowest, flat, np.arange(flat.size))
    rank = np.empty(pts.shape[0], dtype=np.int64)
    rank[np.argsort(lowest)] = np.arange(pts.shape[0])
    return pts[segs], rank[segs].astype(np.int32)


def coincident(S):
    """S segments with every corner at one point."""
    return np.tile(np.array([0.3, 0.7, 0.1]), (S, 2, 1))


# ---------------------------------------------------------------------------------------------------------------------
# real soups
# ---------------------------------------------------------------------------------------------------------------------

def _r2(X):
    return np.sum(X * X, axis=1)


_BLOB_CENTRES = np.array([[-0.5, -0.5, -0.5], [0.5, 0.45, -0.4], [-0.1, 0.5, 0.55]])


def _blobs(X):
    return sum(np.exp(-np.sum((X - c) ** 2, axis=1) / 0.05) for c in _BLOB_CENTRES)


def _cubed_sphere():
    from manifold_twin import cubed_sphere
    return m.fem2d(k=2, K=cubed_sphere(3, k=2), ambient=3)


# name -> (geometry, function of the nodes or None for a tessellation, levels, what to expect)
REAL = {
    "sphere_k1": (lambda: m.subdivide(m.fem3d(k=1), 2), _r2, [0.53], dict(closed=True, chi=[2])),
    "sphere_k2": (lambda: m.subdivide(m.fem3d(k=2), 2), _r2, [0.53], dict(closed=True, chi=[2])),
    "sphere_k3": (lambda: m.subdivide(m.fem3d(k=3), 1), _r2, [0.53], dict(closed=True, chi=[2])),
    "blobs_k2": (lambda: m.subdivide(m.fem3d(k=2), 3), _blobs, [0.3, 0.5, 0.7], dict(closed=True, chi=[2] * 9)),
    "curve_P1": (lambda: m.subdivide(m.fem2d_P1(), 4), _r2, [0.31, 0.62], dict(closed=True, chi=[0, 0])),
    "curve_P2": (lambda: m.subdivide(m.fem2d_P2(), 5), _r2, [0.31, 0.62], dict(closed=True, chi=[0, 0])),
    "curve_k4": (lambda: m.subdivide(m.fem2d(k=4), 3), _r2, [0.31, 0.62], dict(closed=True, chi=[0, 0])),
    "cubed_sphere": (_cubed_sphere, None, None, dict(closed=True, chi=[2])),
}


def real_soup(name, device=False):
    """`(points, group or None, data or None)` of a real soup: from the package on the device, or from the NumPy twins."""
    make, fn, levels, _ = REAL[name]
    geom = make()
    if fn is None:
        fields = geom.xflat[:, 2]
        if device:
            t = m.tessellate(geom, fields)
        else:
            from manifold_twin import tessellate_twin
            t = tessellate_twin(geom, fields.reshape(-1, 1))
        return t.points, None, t.values
    z = fn(geom.xflat)
    carry = geom.xflat[:, 0]
    if device:
        c = m.isocontour(geom, z, levels, carry=carry)
    else:
        from contour_twin import isocontour_twin
        c = isocontour_twin(geom, z, levels, carry=carry)
    return c.points, c.level, c.carried
