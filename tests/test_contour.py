"""isocontour() on the CPU: every argument check raises before the library is touched, an empty `levels` needs no
device, and the NumPy twin (tests/contour_twin.py) the GPU tests compare against is itself checked against exact
answers: linear functions (the cut of a linear function is exact; lengths and areas from polygon clipping) and the
second-order convergence of circles and spheres.  The input condition of the GPU cases (no lattice value within
1024 eps max|z| of a level) is checked here as well, on the twin alone.
"""
import numpy as np
import pytest

import mgb_amd as m
from contour_twin import isocontour_twin, lattice

EPS = float(np.finfo(np.float64).eps)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_contour.py (defined here so that their input condition is checked without a GPU)
# ---------------------------------------------------------------------------------------------------------------------

def _curve(X):
    """A smooth, non-polynomial map of [-1, 1]^2 applied to every node (the idea of tests/test_gpu_locator.py)."""
    Y = X.copy()
    Y[..., 0] += 0.08 * np.sin(np.pi * X[..., 1])
    Y[..., 1] += 0.06 * np.sin(np.pi * X[..., 0]) * X[..., 1]
    return Y


# name -> (geometry, the non-default refine)
GPU_CASES = {
    "fem2d_k1": (lambda: m.subdivide(m.fem2d(k=1), 4), 3),
    "fem2d_k2": (lambda: m.subdivide(m.fem2d(k=2), 3), 5),
    "fem2d_k4": (lambda: m.subdivide(m.fem2d(k=4), 2), 7),
    "fem2d_k2_curved": (lambda: m.fem2d(k=2, K=_curve(m.subdivide(m.fem2d(k=2), 3).x)), 3),
    "fem3d_k1": (lambda: m.subdivide(m.fem3d(k=1), 3), 2),
    "fem3d_k2": (lambda: m.subdivide(m.fem3d(k=2), 2), 3),
    "fem3d_k3": (lambda: m.subdivide(m.fem3d(k=3), 2), 2),
    "fem2d_P1": (lambda: m.subdivide(m.fem2d_P1(), 4), 3),
    "fem2d_P2": (lambda: m.subdivide(m.fem2d_P2(), 3), 5),
    "fem2d_P2_nobubble": (lambda: m.subdivide(m.fem2d_P2(bubble=False), 3), 1),
}
LEVELS5 = np.array([-0.31, -0.12, 0.07, 0.23, 0.41])
LEVELS1 = LEVELS5[2:3]


def smooth(X):
    """A smooth non-polynomial function of the node coordinates, and two more to carry."""
    x, y = X[:, 0], X[:, 1]
    w = X[:, 2] if X.shape[1] == 3 else np.zeros_like(x)
    z = np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2) + 0.35 * np.sin(1.1 * w + 0.3)
    carry = np.stack([np.exp(0.5 * x - 0.3 * y + 0.2 * w), np.cos(x + 2.0 * y - w)], axis=1)
    return z, carry


def input_margin_ok(twin, z):
    """The input condition: no lattice value within 1024 eps max|z| of a level (otherwise two summation orders could
    legitimately classify a lattice point differently)."""
    return twin.margin > 1024 * EPS * float(np.abs(z).max())


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_meet_the_input_condition_on_the_twin(name):
    make, other = GPU_CASES[name]
    geom = make()
    z, _ = smooth(geom.xflat)
    for refine in (None, other):
        t = isocontour_twin(geom, z, LEVELS5, refine=refine)
        print(f"{name} refine={refine}: margin {t.margin:.3e}, S = {t.level.size}")
        assert input_margin_ok(t, z), (name, refine, t.margin)
        assert all((t.level == l).any() for l in range(5)), "every level is meant to cut the mesh"


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: ValueError before any device work
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library or open a device context fails the test."""
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "load_library", boom)
    monkeypatch.setattr(device, "HipContext", boom)


def _n(geom):
    return geom.x.shape[0] * geom.x.shape[1]


def test_isocontour_is_exported():
    from mgb_amd.contour import isocontour, Contour
    assert m.isocontour is isocontour and m.Contour is Contour


@pytest.mark.parametrize("geom,name", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
])
def test_unsupported_families_are_refused_by_name(no_library, geom, name):
    with pytest.raises(ValueError, match=rf"isocontour: {name} geometries are not supported"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0])


def test_embedded_manifold_is_refused(no_library):
    geom = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)     # a segment in the plane
    with pytest.raises(ValueError, match=r"isocontour: fem1d embedded in 2 dimensions"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0])


SUPPORTED = [m.fem2d(k=2), m.fem3d(k=1), m.fem2d_P1(), m.fem2d_P2(), m.fem2d_P2(bubble=False)]


@pytest.mark.parametrize("geom", SUPPORTED)
def test_wrong_shapes_are_refused(no_library, geom):
    n = _n(geom)
    for bad in (np.zeros(n + 1), np.zeros(n - 1), np.zeros((n, 1)), np.zeros((n, 2)), 0.5):
        with pytest.raises(ValueError, match=rf"z must be a vector of {n} values"):
            m.isocontour(geom, bad, [0.0])
    for bad in (np.zeros(n + 1), np.zeros((n - 1, 2)), np.zeros((n, 1, 1)), 0.5):
        with pytest.raises(ValueError, match="carry must be"):
            m.isocontour(geom, np.zeros(n), [0.0], carry=bad)
    for bad in (np.zeros((n, 5)), np.zeros((n, 0))):
        with pytest.raises(ValueError, match=r"carry has \d columns; 1\.\.4 are supported"):
            m.isocontour(geom, np.zeros(n), [0.0], carry=bad)
    with pytest.raises(ValueError, match="levels must be a scalar or a 1-D array"):
        m.isocontour(geom, np.zeros(n), np.zeros((2, 2)))


@pytest.mark.parametrize("geom", SUPPORTED)
def test_refine_out_of_range_is_refused(no_library, geom):
    n, d = _n(geom), geom.x.shape[2]
    top = 16 if d == 2 else 8
    for bad in (0, -1, top + 1):
        with pytest.raises(ValueError, match=rf"refine = {bad} is outside 1\.\.{top}"):
            m.isocontour(geom, np.zeros(n), [0.0], refine=bad)
    for bad in (2.0, "2", True):
        with pytest.raises(ValueError, match="refine must be an integer"):
            m.isocontour(geom, np.zeros(n), [0.0], refine=bad)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_nonfinite_level_is_refused(no_library, bad):
    geom = m.fem2d_P1()
    with pytest.raises(ValueError, match="every level must be finite"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0, bad])
    with pytest.raises(ValueError, match="every level must be finite"):
        m.isocontour(geom, np.zeros(_n(geom)), bad)


@pytest.mark.parametrize("bubble", [True, False])
def test_curved_p2_is_refused(no_library, bubble):
    geom = m.fem2d_P2(bubble=bubble)
    K = geom.x.copy()
    slot = 6 if bubble else 3
    K[slot, 0, 0] += 1e-9 * (1 + abs(K[slot, 0, 0]))
    bent = m.fem2d_P2(bubble=bubble, K=K)
    with pytest.raises(ValueError, match="fem2d_P2 .* straight elements"):
        m.isocontour(bent, np.zeros(_n(bent)), [0.0])


def test_degree_and_mesh_checks(no_library):
    geom = m.fem2d(k=9)
    with pytest.raises(ValueError, match=r"element degree k = 9 is outside 1\.\.8"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0])
    geom = m.fem2d_P1(K=m.fem2d_P1().x.copy())
    geom.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0])


@pytest.mark.parametrize("geom", SUPPORTED)
def test_no_levels_gives_an_empty_result_without_a_device(no_library, geom):
    n, d = _n(geom), geom.x.shape[2]
    for carry in (None, np.zeros(n), np.zeros((n, 3))):
        c = m.isocontour(geom, np.zeros(n), [], carry=carry)
        assert c.points.shape == (0, d, d) and c.points.dtype == np.float64
        assert c.level.shape == (0,) and c.level.dtype == np.int32
        assert c.element.shape == (0,) and c.element.dtype == np.int32
        if carry is None:
            assert c.carried is None
        else:
            assert c.carried.shape == (0, d, np.asarray(carry).reshape(n, -1).shape[1])
        assert c.measure().shape == (0,)


def test_measure_sums_lengths_and_areas_per_level():
    seg = np.array([[[0.0, 0.0], [3.0, 4.0]], [[1.0, 1.0], [1.0, 3.0]], [[0.0, 0.0], [1.0, 0.0]]])
    c = m.Contour(seg, np.array([2, 0, 2], dtype=np.int32), np.zeros(3, dtype=np.int32), None, 4)
    assert np.array_equal(c.measure(), [2.0, 0.0, 6.0, 0.0])
    tri = np.array([[[0.0, 0, 0], [2.0, 0, 0], [0.0, 2, 0]], [[0.0, 0, 1], [0.0, 1, 1], [0.0, 0, 2]]])
    c = m.Contour(tri, np.array([1, 1], dtype=np.int32), np.zeros(2, dtype=np.int32), None, 2)
    assert np.array_equal(c.measure(), [0.0, 2.5])


# ---------------------------------------------------------------------------------------------------------------------
# the twin against exact answers: linear functions
# ---------------------------------------------------------------------------------------------------------------------

def _clip(poly, nrm, off):
    """Sutherland-Hodgman: the part of the polygon `poly` (n, dim) with nrm . x <= off."""
    out = []
    n = len(poly)
    for i in range(n):
        p, q = poly[i], poly[(i + 1) % n]
        sp, sq = nrm @ p - off, nrm @ q - off
        if sp <= 0:
            out.append(p)
        if (sp < 0 < sq) or (sq < 0 < sp):
            out.append(p + (sp / (sp - sq)) * (q - p))
    return np.array(out)


def _line_in_square(a, b, c):
    """Length of {a . x + b = c} inside [-1, 1]^2: the line as a long segment, clipped by the four half-planes."""
    a = np.asarray(a, dtype=np.float64)
    x0 = a * (c - b) / (a @ a)
    t = np.array([-a[1], a[0]]) / np.linalg.norm(a)
    seg = np.array([x0 - 8.0 * t, x0 + 8.0 * t])
    for ax in range(2):
        for s in (1.0, -1.0):
            nrm = np.zeros(2)
            nrm[ax] = s
            # a segment as a degenerate polygon: clip its two ends
            p, q = seg
            sp, sq = nrm @ p - 1.0, nrm @ q - 1.0
            if sp > 0 and sq > 0:
                return 0.0
            if sp > 0:
                p = p + (sp / (sp - sq)) * (q - p)
            if sq > 0:
                q = q + (sq / (sq - sp)) * (p - q)
            seg = np.array([p, q])
    return float(np.linalg.norm(seg[1] - seg[0]))


def _plane_in_cube(a, b, c):
    """Area of {a . x + b = c} inside [-1, 1]^3: a large square of the plane clipped by the six half-spaces."""
    a = np.asarray(a, dtype=np.float64)
    x0 = a * (c - b) / (a @ a)
    u = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.9 * np.linalg.norm(a) else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    v /= np.linalg.norm(v)
    poly = np.array([x0 + 8 * (su * u + sv * v) for su, sv in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    for ax in range(3):
        for s in (1.0, -1.0):
            nrm = np.zeros(3)
            nrm[ax] = s
            poly = _clip(poly, nrm, 1.0)
            if len(poly) < 3:
                return 0.0
    area = np.zeros(3)
    for i in range(1, len(poly) - 1):
        area += np.cross(poly[i] - poly[0], poly[i + 1] - poly[0])
    return 0.5 * float(np.linalg.norm(area))


# (a, b, c): one axis-aligned and one oblique line / plane; neither passes through a lattice point of the meshes below
LINES = [((1.0, 0.0), 0.0, 0.3), ((0.3, -0.7), 0.11, 0.2)]
PLANES = [((0.0, 0.0, 1.0), 0.0, 0.3), ((0.3, -0.7, 0.5), 0.11, 0.2)]
LINEAR = [("fem2d_P1", lambda: m.subdivide(m.fem2d_P1(), 3), LINES),
          ("fem2d_Q1", lambda: m.subdivide(m.fem2d(k=1), 3), LINES),
          ("fem3d_Q1", lambda: m.subdivide(m.fem3d(k=1), 3), PLANES)]


def check_linear(name, geom, contour, a, b, c):
    """The assertions of the linear case on any contour object (the twin here, the device in the GPU tests)."""
    X = geom.xflat
    d = X.shape[1]
    a = np.asarray(a, dtype=np.float64)
    z = X @ a + b
    assert np.array_equal(X.min(axis=0), -np.ones(d)) and np.array_equal(X.max(axis=0), np.ones(d))
    assert abs(float(geom.w.sum()) - 2.0 ** d) < 1e-12          # the default domain is the whole square / cube
    S = contour.level.size
    assert S > 0
    resid = np.abs(contour.points @ a + b - c).max()
    exact = _line_in_square(a, b, c) if d == 2 else _plane_in_cube(a, b, c)
    got = float(contour.measure()[0])
    diam = 2.0 * np.sqrt(d)
    print(f"linear {name} a={tuple(a)}: S = {S}, residual {resid / EPS:.2f} eps, measure {got:.15g} vs {exact:.15g} "
          f"({abs(got - exact) / EPS:.1f} eps, allowed {S * 8 * diam:.0f} eps)")
    assert resid <= 64 * EPS * np.abs(z).max()
    assert abs(got - exact) <= S * 8 * EPS * diam


@pytest.mark.parametrize("name,make,cuts", LINEAR)
def test_twin_cuts_linear_functions_exactly(name, make, cuts):
    geom = make()
    for a, b, c in cuts:
        z = geom.xflat @ np.asarray(a) + b
        t = isocontour_twin(geom, z, [c])
        assert t.margin > 0.0, "the cut is meant to avoid the lattice points"
        check_linear(name, geom, t, a, b, c)


def test_twin_order_vertices_and_shared_bits():
    """Structure of the twin's output: order by element, every vertex on its level within rounding of the lattice
    values, interior vertices shared bit for bit by two simplices of the same element."""
    geom = m.subdivide(m.fem3d(k=2), 2)
    z, carry = smooth(geom.xflat)
    t = isocontour_twin(geom, z, LEVELS5, refine=3, carry=carry)
    assert np.all(np.diff(t.element) >= 0)
    assert t.points.shape == (t.level.size, 3, 3) and t.carried.shape == (t.level.size, 3, 2)
    # each vertex of the soup that is not on an element face occurs in several triangles with identical bits
    e = 0
    P = t.points[(t.element == e) & (t.level == 2)].reshape(-1, 3)
    _, counts = np.unique(P, axis=0, return_counts=True)
    assert counts.max() >= 3 and (counts >= 2).mean() > 0.5
    one = isocontour_twin(geom, z, LEVELS5, refine=3, carry=carry[:, 1])
    assert np.array_equal(one.carried[..., 0], t.carried[..., 1]) and np.array_equal(one.points, t.points)


# ---------------------------------------------------------------------------------------------------------------------
# the twin against exact answers: circles and spheres (second order in the lattice spacing)
# ---------------------------------------------------------------------------------------------------------------------
# Level 0.37 (radius 0.608...): the circle / sphere lies inside [-1, 1]^d and meets no lattice point of the meshes
# below at any of the refinements (margins printed).  Q2 represents x^2 + y^2 (+ z^2) exactly, so the only error is the
# piecewise-linear cut, O(h^2): the error falls by about 4 per doubling of `refine`; the test asks for 2.

def test_twin_circle_length_converges():
    geom = m.subdivide(m.fem2d(k=2), 3)
    X = geom.xflat
    z = X[:, 0] ** 2 + X[:, 1] ** 2
    c = 0.37
    errs = []
    for r in (2, 4, 8):
        t = isocontour_twin(geom, z, [c], refine=r)
        assert t.margin > 1024 * EPS
        errs.append(abs(t.measure()[0] - 2 * np.pi * np.sqrt(c)))
    print("circle length errors at refine 2, 4, 8:", errs)
    assert errs[1] <= errs[0] / 2 and errs[2] <= errs[1] / 2


def test_twin_sphere_area_converges():
    geom = m.subdivide(m.fem3d(k=2), 2)
    z = (geom.xflat ** 2).sum(axis=1)
    c = 0.37
    errs = []
    for r in (2, 4):
        t = isocontour_twin(geom, z, [c], refine=r)
        assert t.margin > 1024 * EPS
        errs.append(abs(t.measure()[0] - 4 * np.pi * c))
    print("sphere area errors at refine 2, 4:", errs)
    assert errs[1] <= errs[0] / 2


def test_twin_lattice_reproduces_the_nodes_at_the_default_refine_of_q1():
    """At refine = k = 1 the lattice of a Q1 element is its nodes: values and positions are the inputs."""
    geom = m.subdivide(m.fem3d(k=1), 2)
    z, _ = smooth(geom.xflat)
    V, X, _, simp = lattice(geom, z)
    p, N, d = geom.x.shape
    assert np.array_equal(V, z.reshape(N, p)) and np.array_equal(X, geom.xflat.reshape(N, p, d))
    assert simp.shape == (6, 4) and np.all(np.diff(simp, axis=1) > 0)
