"""Post-processing of `fem2d` surfaces in R^3 without a GPU: the argument checks of `tessellate`, of `isocontour` on a
surface and of the `render_surfaces` / `render_figure` branches that take one, and the NumPy twin
(tests/manifold_twin.py) against `isocontour_twin`, against exact answers on the cubed sphere and on a tilted plane.  The
cases of tests/test_gpu_manifold_post.py are defined here so that their input condition is checked without a GPU."""
import numpy as np
import pytest

import mgb_amd as m
from contour_twin import isocontour_twin
from manifold_twin import cubed_sphere, isocontour_twin_e, tessellate_twin
from mgb_amd.contour import Contour, Tessellation
from mgb_amd.surface import render_figure, render_surfaces
from test_contour import EPS, LEVELS1, LEVELS5, _curve, input_margin_ok, smooth


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_manifold_post.py
# ---------------------------------------------------------------------------------------------------------------------

def sphere(mm, k=1):
    """The cubed sphere of the reference's test/test_manifold.jl: 6 mm^2 Q_k quads, every node on the unit sphere."""
    return m.fem2d(k=k, K=cubed_sphere(mm, k), ambient=3)


SURFACE_CASES = {
    "sphere_m1_k1": lambda: sphere(1, 1),
    "sphere_m2_k1": lambda: sphere(2, 1),
    "sphere_m1_k2": lambda: sphere(1, 2),
    "sphere_m1_k4": lambda: sphere(1, 4),
}
REFINES = (None, 3, 8, 9, 16)       # 8 | 9: one wave | a workgroup of four; 16: the cap
# flat families of tessellate: (geometry, the refine besides the default)
FLAT_CASES = {
    "fem2d_k2": (lambda: m.subdivide(m.fem2d(k=2), 2), 3),
    "fem2d_P1": (lambda: m.subdivide(m.fem2d_P1(), 2), 3),
    "fem2d_P2": (lambda: m.subdivide(m.fem2d_P2(), 2), 5),
}


def flat_pair(k):
    """A 4 x 4 `fem2d` mesh in R^2 (curved for k = 2) and the same nodes with a third coordinate of exactly 0.0 in R^3."""
    g2 = m.subdivide(m.fem2d(k=k), 3)                      # 16 elements
    assert g2.x.shape[1] == 16
    if k == 2:
        g2 = m.fem2d(k=2, K=_curve(g2.x))
    K3 = np.concatenate([g2.x, np.zeros(g2.x.shape[:2] + (1,))], axis=2)
    return g2, m.fem2d(k=k, K=K3, ambient=3)


@pytest.mark.parametrize("name", sorted(SURFACE_CASES))
def test_gpu_cases_meet_the_input_condition_on_the_twin(name):
    geom = SURFACE_CASES[name]()
    z, _ = smooth(geom.xflat)
    for refine in REFINES:
        t = isocontour_twin_e(geom, z, LEVELS5, refine=refine)
        print(f"{name} refine={refine}: margin {t.margin:.3e}, S = {t.level.size}")
        assert input_margin_ok(t, z), (name, refine, t.margin)
        assert t.level.size > 0 and np.any(t.level == 2)            # LEVELS1 is LEVELS5[2]
    for k in (1, 2):
        g2, _ = flat_pair(k)
        z2, _ = smooth(g2.xflat)
        assert isocontour_twin_e(g2, z2, LEVELS5).level.size > 0


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: all before any device work
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


def test_tessellate_is_exported():
    from mgb_amd.contour import tessellate
    assert m.tessellate is tessellate and m.Tessellation is Tessellation


CURVE2 = lambda: m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)          # noqa: E731
CURVE3 = lambda: m.fem1d(K=np.array([[[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]]]), ambient=3)  # noqa: E731


@pytest.mark.parametrize("make,e", [(CURVE2, 2), (CURVE3, 3)])
def test_curves_are_still_refused_with_the_old_text(no_library, make, e):
    geom = make()
    with pytest.raises(ValueError, match=rf"^isocontour: fem1d embedded in {e} dimensions \(a manifold\) is not supported$"):
        m.isocontour(geom, np.zeros(_n(geom)), [0.0])
    with pytest.raises(ValueError, match=rf"^tessellate: fem1d embedded in {e} dimensions \(a manifold\) is not supported$"):
        m.tessellate(geom)
    with pytest.raises(ValueError, match=rf"^render_figure: fem1d embedded in {e} dimensions \(a manifold\) is not supported$"):
        render_figure(geom, np.zeros(_n(geom)), (0, -4, 0), (0, 0, 0))


@pytest.mark.parametrize("geom,name", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.fem3d(k=1), "fem3d"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
])
def test_tessellate_refuses_other_families_by_name(no_library, geom, name):
    with pytest.raises(ValueError, match=rf"tessellate: {name} geometries are not supported"):
        m.tessellate(geom)


def test_tessellate_argument_checks(no_library):
    g = sphere(1, 2)
    n = _n(g)
    for fields, kw, match in [
        (np.zeros(n + 1), {}, rf"fields must be \({n},\) or \({n}, nfield\) for this fem2d geometry"),
        (np.zeros((n, 2, 1)), {}, r"fields must be"),
        (np.zeros((n, 6)), {}, r"fields has 6 columns; 1\.\.5 are supported"),
        (np.zeros((n, 0)), {}, r"fields has 0 columns; 1\.\.5 are supported"),
        (None, dict(refine=0), r"refine = 0 is outside 1\.\.16 for 2-D elements"),
        (None, dict(refine=17), r"refine = 17 is outside 1\.\.16 for 2-D elements"),
        (None, dict(refine=2.0), r"refine must be an integer"),
        (None, dict(refine=True), r"refine must be an integer"),
    ]:
        with pytest.raises(ValueError, match="tessellate: " + match):
            m.tessellate(g, fields, **kw)
    bad = m.fem2d(k=1, K=cubed_sphere(1, 1), ambient=3)
    bad.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="tessellate: the fem2d mesh has non-finite node coordinates"):
        m.tessellate(bad)
    for make in (lambda: sphere(1, 1), m.fem2d, m.fem2d_P1):
        g0 = make()
        empty = m.Geometry(g0.discretization, g0.t[:, :0], g0.x[:, :0], g0.w[:0], g0.operators)
        with pytest.raises(ValueError, match=r"tessellate: the fem2d\w* geometry has no elements"):
            m.tessellate(empty)


def test_isocontour_on_a_surface_argument_checks(no_library):
    g = sphere(1, 1)
    n = _n(g)
    z = g.xflat[:, 2].copy()
    for args, kw, match in [
        ((np.zeros(n + 1), [0.0]), {}, rf"z must be a vector of {n} values for this fem2d geometry"),
        ((z, [0.0]), dict(carry=np.zeros(n - 1)), rf"carry must be \({n},\) or \({n}, ncarry\)"),
        ((z, [0.0]), dict(carry=np.zeros((n, 5))), r"carry has 5 columns; 1\.\.4 are supported"),
        ((z, [np.inf]), {}, "every level must be finite"),
        ((z, [0.0]), dict(refine=17), r"refine = 17 is outside 1\.\.16 for 2-D elements"),
        ((z, [0.0]), dict(refine=1.5), "refine must be an integer"),
    ]:
        with pytest.raises(ValueError, match="isocontour: " + match):
            m.isocontour(g, *args, **kw)
    g.x[0, 0, 0] = np.inf
    with pytest.raises(ValueError, match="isocontour: the fem2d mesh has non-finite node coordinates"):
        m.isocontour(g, z, [0.0])
    # no levels: an empty result in R^3 without touching the device
    c = m.isocontour(sphere(1, 1), z, [])
    assert c.points.shape == (0, 2, 3) and c.carried is None and c.measure().shape == (0,)


def test_interpolate_still_refuses_surfaces(no_library):
    g = sphere(1, 1)
    with pytest.raises(ValueError, match="interpolate: embedded manifolds"):
        m.interpolate(g, np.zeros(_n(g)), np.zeros((1, 3)))


def test_render_surfaces_tessellation_refusals(no_library):
    cam = dict(eye=(0, -4, 0), target=(0, 0, 0), size=(4, 3))
    flat = Tessellation(np.zeros((1, 3, 2)), np.zeros(1, np.int32), np.ones((1, 3, 1)))
    bare = Tessellation(np.zeros((1, 3, 3)), np.zeros(1, np.int32), None)
    tri = Contour(np.zeros((1, 3, 3)), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1)
    with pytest.raises(ValueError, match=r"render_surfaces: a Tessellation must be of a surface in R\^3.*e = 2"):
        render_surfaces(flat, **cam)
    with pytest.raises(ValueError, match=r"render_surfaces: a Tessellation without values needs values="):
        render_surfaces(bare, **cam)
    with pytest.raises(ValueError, match=r"render_surfaces: a Tessellation without values needs values="):
        render_surfaces([tri, bare], levels=[[0.5], None], **cam)
    with pytest.raises(ValueError, match=r"render_surfaces: values must be \(2,\) or \(2, 3\)"):
        render_surfaces([tri, bare], values=np.zeros(3), **cam)
    with pytest.raises(ValueError, match="render_surfaces: contours must be a Contour or a list of them"):
        render_surfaces([bare, 3], **cam)


def test_render_figure_on_a_surface_refusals(no_library):
    g = sphere(1, 1)
    u = g.xflat[:, 2].copy()
    cam = dict(eye=(0, -4, 0), target=(0, 0, 0), size=(4, 3))
    for kw, match in [
        (dict(isosurfaces=[0.1]), r"isosurfaces has no meaning for a fem2d surface in R\^3"),
        (dict(isosurfaces=[]), r"isosurfaces has no meaning for a fem2d surface in R\^3"),
        (dict(slices=[(0, 0.1)]), r"slices has no meaning for a fem2d surface in R\^3"),
        (dict(volume=True), r"volume=True has no meaning for a fem2d surface in R\^3"),
        (dict(step=0.1), r"step has no meaning for a fem2d surface in R\^3"),
        (dict(refine=17), r"refine = 17 is outside 1\.\.16"),
        (dict(refine=1.5), r"refine must be an integer"),
        (dict(size=(0, 3)), "size"),
        (dict(clim=(1.0, 1.0)), "clim must be finite with lo < hi"),
        (dict(surface_alpha=2), r"surface_alpha must be a number in \[0, 1\]"),
        (dict(ambient=-1), "ambient must be a number"),
        (dict(transfer=np.zeros((2, 3))), r"transfer must be \(K, 4\)"),
    ]:
        with pytest.raises(ValueError, match=match):
            render_figure(g, u, **{**cam, **kw})
    with pytest.raises(ValueError, match=rf"render_figure: u must be a vector of {_n(g)} values for this fem2d geometry"):
        render_figure(g, u[:-1], **cam)
    # refine belongs to surfaces
    g3 = m.fem3d(k=1)
    with pytest.raises(ValueError, match="render_figure: refine is for a fem2d surface"):
        render_figure(g3, np.arange(8.0), refine=2, **cam)


# ---------------------------------------------------------------------------------------------------------------------
# measures
# ---------------------------------------------------------------------------------------------------------------------

def test_measures():
    rng = np.random.default_rng(3)
    P2 = rng.standard_normal((7, 2, 2))
    c2 = Contour(P2, np.zeros(7, np.int32), np.zeros(7, np.int32), None, 1)
    old = np.hypot(P2[:, 1, 0] - P2[:, 0, 0], P2[:, 1, 1] - P2[:, 0, 1])
    assert np.array_equal(c2.measure(), np.bincount(np.zeros(7, np.int32), weights=old, minlength=1))     # bitwise
    P3 = np.array([[[0.0, 0.0, 0.0], [1.0, 2.0, 2.0]], [[1.0, 1.0, 1.0], [1.0, 4.0, 5.0]]])
    c3 = Contour(P3, np.array([0, 1], np.int32), np.zeros(2, np.int32), None, 2)
    assert np.array_equal(c3.measure(), [3.0, 5.0])
    t3 = Tessellation(np.array([[[0.0, 0, 0], [2.0, 0, 0], [0.0, 0, 3.0]]]), np.zeros(1, np.int32), None)
    t2 = Tessellation(np.array([[[0.0, 0], [0.0, 3.0], [2.0, 0]], [[0.0, 0], [1.0, 0], [0.0, 1.0]]]), np.zeros(2, np.int32), None)
    assert t3.measure() == 3.0 and t2.measure() == 3.5 and isinstance(t3.measure(), float)


# ---------------------------------------------------------------------------------------------------------------------
# the twin
# ---------------------------------------------------------------------------------------------------------------------

def test_twin_with_two_coordinates_is_the_contour_twin_bitwise():
    g = m.fem2d(k=2, K=_curve(m.subdivide(m.fem2d(k=2), 2).x))
    z, carry = smooth(g.xflat)
    a = isocontour_twin(g, z, LEVELS5, refine=3, carry=carry)
    b = isocontour_twin_e(g, z, LEVELS5, refine=3, carry=carry)
    assert a.level.size > 0
    for f in ("points", "level", "element", "carried", "dv", "dx", "dc"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), f
    assert a.margin == b.margin and np.array_equal(a.measure(), b.measure())


def test_twin_embedding_independence():
    for k in (1, 2):
        g2, g3 = flat_pair(k)
        z, carry = smooth(g2.xflat)
        a = isocontour_twin_e(g2, z, LEVELS5, refine=3, carry=carry)
        b = isocontour_twin_e(g3, z, LEVELS5, refine=3, carry=carry)
        assert np.array_equal(b.points[..., :2], a.points) and np.all(b.points[..., 2] == 0.0)
        assert np.array_equal(a.carried, b.carried) and np.array_equal(a.level, b.level)
        ta, tb = tessellate_twin(g2, z, 3), tessellate_twin(g3, z, 3)
        assert np.array_equal(tb.points[..., :2], ta.points) and np.all(tb.points[..., 2] == 0.0)
        assert np.array_equal(ta.values, tb.values)
        assert abs(ta.measure() - 4.0) < (1e-12 if k == 1 else 0.05) and ta.measure() == tb.measure()


def test_twin_contour_vertices_lie_on_tessellation_edges_bitwise():
    g = sphere(2, 1)
    z, _ = smooth(g.xflat)
    c = isocontour_twin_e(g, z, LEVELS5, refine=3)
    t = tessellate_twin(g, z, refine=3)
    i = c.tri[:, None]
    va, vb = t.values[i, c.qa, 0], t.values[i, c.qb, 0]
    xa, xb = t.points[i, c.qa], t.points[i, c.qb]
    tt = (LEVELS5[c.level][:, None] - va) / (vb - va)
    assert np.array_equal(xa + tt[..., None] * (xb - xa), c.points)
    assert np.array_equal(t.element[c.tri], c.element)


C037 = 0.37
LENGTH = 2.0 * np.pi * np.sqrt(1.0 - C037 * C037)
AREA = 4.0 * np.pi


def _sphere_errors(mm, k):
    g = sphere(mm, k)
    c = isocontour_twin_e(g, g.xflat[:, 2].copy(), [C037])
    t = tessellate_twin(g)
    return abs(t.measure() - AREA), abs(float(c.measure()[0]) - LENGTH)


@pytest.mark.parametrize("k,ms", [(1, (4, 8, 16)), (2, (2, 4, 8))], ids=["q1_corners", "k2_all_nodes"])
def test_twin_on_the_cubed_sphere_is_second_order(k, ms):
    """The level curve {x_3 = 0.37} has length 2 pi sqrt(1 - 0.37^2) and the sphere area 4 pi; both errors are second
    order in the lattice spacing, so a doubling of m divides them by 4 asymptotically: at least 3 is asserted.

    The doubling is of m, at the default `refine`.  A doubling of `refine` on a fixed mesh converges to the length and
    area of the Q_k surface, which is not the sphere (its nodes are on it, the rest is not), so it is not compared with
    the sphere's.  The smallest sizes are not asymptotic for the length (Q1: m = 1 -> 2 gives 2.30, 2 -> 4 gives 5.36),
    so the doublings start at m = 4 (Q1) and m = 2 (k = 2: the same lattice points as Q1 with 2 m).  Observed: area
    3.84, 3.96; length 3.05, 3.92."""
    errs = [_sphere_errors(mm, k) for mm in ms]
    for (a0, l0), (a1, l1), mm in zip(errs, errs[1:], ms):
        print(f"cubed sphere k={k} m={mm}->{2 * mm}: area error {a0:.3e} -> {a1:.3e} (factor {a0 / a1:.2f}), "
              f"length error {l0:.3e} -> {l1:.3e} (factor {l0 / l1:.2f})")
        assert a0 / a1 >= 3.0 and l0 / l1 >= 3.0


def test_twin_is_exact_on_a_tilted_plane():
    """The unit square mesh rotated into a tilted plane of R^3, z linear in the in-plane coordinates: every emitted point
    lies on the exact line to 64 eps max|x| and the total length is the clipped line's."""
    g2 = m.subdivide(m.fem2d(k=2), 3)                      # [-1, 1]^2, 4 x 4 elements
    assert g2.x.shape[1] == 16
    s, t = g2.xflat[:, 0], g2.xflat[:, 1]
    # an orthonormal frame (u, v) of a tilted plane through x0
    u = np.array([2.0, 1.0, 2.0]) / 3.0
    v = np.array([-2.0, 2.0, 1.0]) / 3.0
    x0 = np.array([0.3, -0.2, 0.5])
    X3 = x0[None, :] + s[:, None] * u[None, :] + t[:, None] * v[None, :]
    g3 = m.fem2d(k=2, K=X3.reshape(g2.x.shape[1], g2.x.shape[0], 3).transpose(1, 0, 2), ambient=3)
    assert np.array_equal(g3.xflat, X3)
    a, b, c0 = 0.8, -0.45, 0.11                            # z = a s + b t; the line a s + b t = c0
    z = a * s + b * t
    for refine in (None, 3):
        c = isocontour_twin_e(g3, z, [c0], refine=refine, carry=s)
        assert c.level.size > 0
        tol = 64 * EPS * float(np.abs(X3).max())
        P = c.points.reshape(-1, 3) - x0
        ps, pt = P @ u, P @ v                               # in-plane coordinates of the emitted points
        assert np.abs(P - ps[:, None] * u - pt[:, None] * v).max() <= tol          # in the plane
        assert np.abs(a * ps + b * pt - c0).max() / np.hypot(a, b) <= tol           # distance to the line
        assert np.abs(c.carried.reshape(-1) - ps).max() <= tol
        # the line a s + b t = c0 clipped to [-1, 1]^2: t runs over [-1, 1] (|b| < |a|: s = (c0 - b t) / a stays inside)
        assert abs((c0 + abs(b)) / a) < 1
        exact = 2.0 * np.sqrt(1.0 + (b / a) ** 2)
        assert abs(float(c.measure()[0]) - exact) <= 64 * EPS * exact
        tess = tessellate_twin(g3, z, refine)
        assert abs(tess.measure() - 4.0) <= 64 * EPS * 4.0
        assert np.abs(tess.values[..., 0] - ((tess.points - x0) @ u * a + (tess.points - x0) @ v * b)).max() <= tol
