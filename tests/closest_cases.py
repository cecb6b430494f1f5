"""The cases tests/test_closest.py (CPU, on the NumPy twin) and tests/test_gpu_closest.py (device against the twin) share:
embedded curves and surfaces, query points at a known offset along a unit normal from a known reference point, and the
special points (out of reach, outside the grid, non-finite, beyond an open end, at a polygon vertex, at the centre).
Every seed is fixed, and a case's twin is computed once per process."""
import functools

import numpy as np

import mgb_amd as m
from closest_twin import basis, closest_twin, default_max_distance
from manifold_twin import cubed_sphere
from mgb_amd.tensorfem import _tf_nodes
from test_manifold_post import flat_pair, sphere
from test_tubes import circle3

DEGREES = (1, 2, 3, 8)
FAR_SCALE, FAR_SHIFT = 1e-3, 1000.0
OFFSET = 0.05                    # |delta| <= OFFSET * the mesh's radius
XI_BOUND = 0.9                   # |xi0| <= XI_BOUND for the parity cases
XI_CLOSED = 0.8                  # ... and the closed forms are asserted where |xi0| <= XI_CLOSED
BLOCK_EDGES = (1, 255, 256, 257)


def _far():
    g = sphere(2, 2)
    return m.fem2d(k=2, K=FAR_SCALE * g.x + FAR_SHIFT, ambient=3)


MESHES = {
    **{f"circle3_k{k}": (lambda k=k: m.fem1d(k=k, K=circle3(8, k), ambient=3)) for k in DEGREES},
    **{f"circle2_k{k}": (lambda k=k: m.fem1d(k=k, K=circle3(8, k)[..., :2].copy(), ambient=2)) for k in DEGREES},
    "arc3_k2": lambda: m.fem1d(k=2, K=circle3(8, 2)[:, :3].copy(), ambient=3),
    "arc2_k3": lambda: m.fem1d(k=3, K=circle3(8, 3)[:, :3, :2].copy(), ambient=2),
    **{f"sphere_m1_k{k}": (lambda k=k: sphere(1, k)) for k in DEGREES},
    "sphere_m2_k2": lambda: sphere(2, 2),
    "flat_k1": lambda: flat_pair(1)[1],
    "flat_k2": lambda: flat_pair(2)[1],
    "one_curve2": lambda: m.fem1d(k=2, K=circle3(8, 2)[:, :1, :2].copy(), ambient=2),
    "one_curve3": lambda: m.fem1d(k=3, K=circle3(8, 3)[:, :1].copy(), ambient=3),
    "one_surface": lambda: m.fem2d(k=2, K=cubed_sphere(1, 2)[:, :1].copy(), ambient=3),
    "far": _far,
}
CURVES = tuple(n for n in MESHES if n.startswith(("circle", "arc", "one_curve")))
CIRCLES = tuple(n for n in MESHES if n.startswith("circle"))

# name -> (mesh, M, seed): the parity cases.  Every mesh at M = 257; the BLOCK edges on the two-level sphere
CASES = {name: (name, 257, 100 + i) for i, name in enumerate(MESHES)}
CASES.update({f"sphere_m2_k2_M{M}": ("sphere_m2_k2", M, 200 + M) for M in BLOCK_EDGES if M != 257})


@functools.lru_cache(maxsize=None)
def mesh(name):
    return MESHES[name]()


def mesh_box(geom):
    X = geom.xflat
    return X.min(axis=0), X.max(axis=0)


def mesh_diagonal(geom) -> float:
    lo, hi = mesh_box(geom)
    return float(np.linalg.norm(hi - lo))


def mesh_radius(geom) -> float:
    return 0.5 * mesh_diagonal(geom)


def element_frame(geom, el, xi0):
    """(x (M, e), J (M, e, d)) of elements `el` at reference points xi0 (M, d)."""
    p, N, e = geom.x.shape
    phi, dphi, _ = basis(_tf_nodes(geom.discretization.k), np.asarray(xi0, dtype=np.float64))
    X = np.asarray(geom.xflat, dtype=np.float64).reshape(N, p, e)[el]
    return np.einsum("bp,bpa->ba", phi, X), np.einsum("bdp,bpa->bad", dphi, X)


def offset_points(geom, M, seed, bound=XI_BOUND):
    """(points (M, e), element, xi0 (M, d), delta (M,), nu (M, e)): x_elem(xi0) + delta nu with nu a unit normal."""
    rng = np.random.default_rng(seed)
    p, N, e = geom.x.shape
    d = geom.discretization.d
    el = rng.integers(0, N, size=M)
    xi0 = rng.uniform(-bound, bound, size=(M, d))
    x0, J = element_frame(geom, el, xi0)
    if d == 2:
        nu = np.cross(J[:, :, 0], J[:, :, 1])
    elif e == 2:
        nu = np.stack([-J[:, 1, 0], J[:, 0, 0]], axis=1)
    else:
        tt = J[:, :, 0]
        v = rng.standard_normal((M, 3))
        nu = v - (np.sum(v * tt, axis=1) / np.sum(tt * tt, axis=1))[:, None] * tt
    nu = nu / np.linalg.norm(nu, axis=1)[:, None]
    delta = rng.uniform(-1.0, 1.0, size=M) * OFFSET * mesh_radius(geom)
    return x0 + delta[:, None] * nu, el, xi0, delta, nu


@functools.lru_cache(maxsize=None)
def case(name):
    """(geom, points, element, xi0, delta, nu) of a parity case."""
    mname, M, seed = CASES[name]
    geom = mesh(mname)
    return (geom,) + offset_points(geom, M, seed)


@functools.lru_cache(maxsize=None)
def case_twin(name):
    geom, pts = case(name)[:2]
    return closest_twin(geom, pts)


def affine_field(geom, seed=7):
    """(z, a, b): z = a . x + b on the nodes."""
    rng = np.random.default_rng(seed)
    e = geom.x.shape[2]
    a, b = rng.uniform(-1.0, 1.0, size=e), 0.3
    return geom.xflat @ a + b, a, b


def smooth_fields(geom):
    """(p*N, 3): smooth non-polynomial functions of the node coordinates, of very different sizes."""
    lo, hi = mesh_box(geom)
    U = (geom.xflat - lo) / max(float((hi - lo).max()), 1e-300)          # the far mesh gets the same fields
    x, y = U[:, 0], U[:, 1]
    w = U[:, 2] if U.shape[1] == 3 else np.zeros_like(x)
    return np.stack([np.sin(2.3 * x + 0.4) * np.cos(1.9 * y - 0.2) + 0.35 * np.sin(2.1 * w + 0.3),
                     1e3 * np.exp(0.5 * x - 0.3 * y + 0.2 * w), 1e-3 * np.cos(x + 2.0 * y - w)], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# special points: name -> (mesh, points, max_distance or None)
# ---------------------------------------------------------------------------------------------------------------------

def _without(mname):
    """Three points without a foot: out of reach but inside the grid box, outside the grid box, and far away."""
    geom = mesh(mname)
    lo, hi = mesh_box(geom)
    md = default_max_distance(geom)
    x0, J = element_frame(geom, np.array([0]), np.zeros((1, geom.discretization.d)))
    c = 0.5 * (lo + hi)
    inward = (c - x0[0]) / np.linalg.norm(c - x0[0])
    return np.stack([x0[0] + 3.0 * md * inward, hi + 4.0 * md, hi + 10.0 * (hi - lo) + 1.0])


def _nonfinite(mname):
    geom = mesh(mname)
    e = geom.x.shape[2]
    base = geom.xflat[0]
    pts = np.tile(base, (3 * e, 1))
    for a in range(e):
        pts[3 * a, a], pts[3 * a + 1, a], pts[3 * a + 2, a] = np.nan, np.inf, -np.inf
    return pts


def _flat_outside(k):
    """In-plane points outside the open square [-1, 1]^2 of flat_pair, and one above its edge."""
    return np.array([[1.04, 0.3, 0.0], [-1.03, -0.55, 0.0], [0.2, 1.05, 0.0], [1.03, 1.02, 0.0], [1.02, 0.1, 0.03]])


def _arc_ends(mname):
    """Points beyond both ends of the open arc, along the end tangents (and one a little off the tangent)."""
    geom = mesh(mname)
    N = geom.x.shape[1]
    x, J = element_frame(geom, np.array([0, N - 1]), np.array([[-1.0], [1.0]]))
    tt = J[:, :, 0] / np.linalg.norm(J[:, :, 0], axis=1)[:, None]
    h = 0.04 * mesh_radius(geom)
    off = np.zeros(geom.x.shape[2])
    off[-1] = 0.3 * h
    return np.stack([x[0] - h * tt[0], x[1] + h * tt[1], x[0] - h * tt[0] + off, x[1] + 0.5 * h * tt[1] - off])


def _vertices(mname):
    """Points on the convex side of every vertex of the k = 1 polygon: the vertex pushed outward along its own direction
    from the polygon's centre."""
    geom = mesh(mname)
    V = geom.x[0]                                                     # (N, e): the first node of every element
    c = V.mean(axis=0)
    return c + 1.04 * (V - c)


def _centre(mname):
    geom = mesh(mname)
    return np.zeros((1, geom.x.shape[2]))


SPECIAL = {
    **{f"without_{n}": (n, lambda n=n: _without(n), None) for n in ("circle3_k2", "circle2_k3", "sphere_m2_k2", "far")},
    **{f"nonfinite_{n}": (n, lambda n=n: _nonfinite(n), None) for n in ("circle2_k2", "sphere_m1_k3")},
    "flat_outside_k1": ("flat_k1", lambda: _flat_outside(1), None),
    "flat_outside_k2": ("flat_k2", lambda: _flat_outside(2), None),
    "arc3_ends": ("arc3_k2", lambda: _arc_ends("arc3_k2"), None),
    "arc2_ends": ("arc2_k3", lambda: _arc_ends("arc2_k3"), None),
    "vertex_circle3_k1": ("circle3_k1", lambda: _vertices("circle3_k1"), None),
    "vertex_circle2_k1": ("circle2_k1", lambda: _vertices("circle2_k1"), None),
    **{f"centre_{n}": (n, lambda n=n: _centre(n), 2.0) for n in CIRCLES},
}
NO_FOOT = tuple(n for n in SPECIAL if n.startswith(("without", "nonfinite")))
CLAMPED = ("flat_outside_k1", "flat_outside_k2", "arc3_ends", "arc2_ends", "vertex_circle3_k1", "vertex_circle2_k1")
DISTANCE_ONLY = tuple(n for n in SPECIAL if n.startswith(("vertex", "centre")))


@functools.lru_cache(maxsize=None)
def special(name):
    """(geom, points, max_distance, twin)."""
    mname, pts, md = SPECIAL[name]
    geom, P = mesh(mname), pts()
    return geom, P, md, closest_twin(geom, P, max_distance=md)


