"""closest_point / ClosestPointLocator on the CPU: every argument check raised before the library is touched, the locator
of zero points without a device, and the NumPy twin (tests/closest_twin.py) the GPU tests compare against, itself pinned
on closed forms.  The cases of tests/test_gpu_closest.py live in tests/closest_cases.py; the input condition their
comparisons rely on (every twin solve converges, hardly any point is equally near two elements) is checked here, on the
twin alone."""
import numpy as np
import pytest

import mgb_amd as m
from closest_cases import (CASES, CURVES, SPECIAL, XI_CLOSED, affine_field, case, case_twin, element_frame, mesh, special)
from closest_twin import DEVICE_MAXIT, default_max_distance
from mgb_amd.closest import ClosestPointLocator, closest_point
from test_manifold_post import no_library, sphere  # noqa: F401  (fixture)
from test_tubes import circle3

# the meshes whose closed forms are asserted at 1e-12: all but the one a thousand units from the origin, whose node
# coordinates carry a rounding error of 1e-13, 1e-10 of the mesh's size
CLOSED = tuple(n for n in CASES if not n.startswith("far"))


def test_the_module_is_exported():
    assert m.closest_point is closest_point and m.ClosestPointLocator is ClosestPointLocator


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: all before any device work
# ---------------------------------------------------------------------------------------------------------------------

def _n(geom):
    return geom.x.shape[0] * geom.x.shape[1]


@pytest.mark.parametrize("geom,match", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), r"fem1d with d = e = 1 is a flat mesh.*use interpolate\(\)"),
    (m.fem2d(k=1), r"fem2d with d = e = 2 is a flat mesh.*use interpolate\(\)"),
    (m.fem3d(k=1), r"fem3d with d = e = 3 is a flat mesh.*use interpolate\(\)"),
    (m.fem2d_P1(), r"no method for FEM2D_P1 geometries"),
    (m.fem2d_P2(), r"no method for FEM2D_P2 geometries"),
    (m.spectral1d(n=4), r"no method for SPECTRAL1D geometries"),
    (m.spectral2d(n=4), r"no method for SPECTRAL2D geometries"),
])
def test_other_geometries_are_refused(no_library, geom, match):  # noqa: F811
    e = geom.x.shape[2]
    with pytest.raises(ValueError, match="closest_point: " + match):
        closest_point(geom, np.zeros(_n(geom)), np.zeros((2, e)))
    with pytest.raises(ValueError, match="closest_point: " + match):
        ClosestPointLocator(geom, np.zeros((2, e)))


def test_interpolate_still_refuses_manifolds(no_library):  # noqa: F811
    g = sphere(1, 1)
    with pytest.raises(ValueError, match="embedded manifolds"):
        m.interpolate(g, np.zeros(_n(g)), np.zeros((1, 3)))


def test_argument_checks(no_library):  # noqa: F811
    g = sphere(1, 2)
    n = _n(g)
    ok = np.zeros((3, 3))
    for t, kw, match in [
        (np.zeros((3, 2)), {}, r"the points must form an M-by-3 array \(got shape \(3, 2\)\)"),
        (np.zeros(2), {}, r"the points must form an M-by-3 array"),
        (np.zeros((2, 3, 1)), {}, r"the points must form an M-by-3 array"),
        (ok, dict(max_distance=-1e-3), r"max_distance = -0\.001 must be finite and >= 0"),
        (ok, dict(max_distance=np.inf), r"max_distance = inf must be finite and >= 0"),
        (ok, dict(max_distance=np.nan), r"max_distance = nan must be finite and >= 0"),
        (ok, dict(max_distance="1"), r"max_distance must be a number or None"),
        (ok, dict(max_distance=True), r"max_distance must be a number or None"),
    ]:
        with pytest.raises(ValueError, match="closest_point: " + match):
            ClosestPointLocator(g, t, **kw)
        with pytest.raises(ValueError, match="closest_point: " + match):
            closest_point(g, np.zeros(n), t, **kw)
    g9 = m.fem1d(k=9, K=circle3(4, 9), ambient=3)
    with pytest.raises(ValueError, match=r"closest_point: element degree k = 9 is outside 1\.\.8"):
        ClosestPointLocator(g9, np.zeros((1, 3)))
    bad = sphere(1, 1)
    bad.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="closest_point: the fem2d mesh has non-finite node coordinates"):
        ClosestPointLocator(bad, ok)
    g0 = sphere(1, 1)
    empty = m.Geometry(g0.discretization, g0.t[:, :0], g0.x[:, :0], g0.w[:0], g0.operators)
    with pytest.raises(ValueError, match="closest_point: the fem2d geometry has no elements"):
        ClosestPointLocator(empty, ok)


def test_zero_points_need_no_library(no_library):  # noqa: F811
    for g in (sphere(1, 2), mesh("circle2_k3")):
        e, n = g.x.shape[2], _n(g)
        with ClosestPointLocator(g, np.zeros((0, e))) as cp:
            assert cp.n_points == 0 and cp.max_distance == default_max_distance(g)
            assert cp.elements.shape == (0,) and cp.elements.dtype == np.int32
            assert cp.xi.shape == (0, g.discretization.d) and cp.points.shape == (0, e)
            assert cp.distances.shape == (0,) and cp.converged.shape == (0,) and cp.converged.dtype == bool
            assert cp.evaluate(np.zeros(n)).shape == (0,)
            assert cp.evaluate(np.zeros((n, 2))).shape == (0, 2)
            v, gr = cp.evaluate(np.zeros((n, 2)), gradient=True)
            assert v.shape == (0, 2) and gr.shape == (0, 2, e)
            with pytest.raises(ValueError, match=rf"needs {n} values \(got {n + 1}\)"):
                cp.evaluate(np.zeros(n + 1))
            with pytest.raises(ValueError, match="z must be a vector or a matrix"):
                cp.evaluate(np.zeros((n, 1, 1)))
        with pytest.raises(ValueError, match="^ClosestPointLocator: the locator is closed$"):
            cp.evaluate(np.zeros(n))
        with pytest.raises(ValueError, match="^ClosestPointLocator: the locator is closed$"):
            cp.elements
        cp.close()
        v, el, di = closest_point(g, np.zeros(n), np.zeros((0, e)), return_element=True, return_distance=True)
        assert v.shape == (0,) and el.shape == (0,) and di.shape == (0,)


def test_the_default_max_distance_is_an_eighth_of_the_largest_element_diagonal():
    g = m.fem1d(k=1, K=np.array([[[0.0, 0.0], [5.0, 5.0]], [[3.0, 4.0], [5.0, 6.0]]]), ambient=2)
    assert default_max_distance(g) == 0.125 * 5.0
    from mgb_amd.closest import default_max_distance as product
    for name in ("sphere_m2_k2", "circle3_k8", "far"):
        assert product(mesh(name)) == default_max_distance(mesh(name))


# ---------------------------------------------------------------------------------------------------------------------
# the twin against closed forms
# ---------------------------------------------------------------------------------------------------------------------

def _closed_subset(name):
    geom, pts, el, xi0, delta, nu = case(name)
    return geom, el, xi0, delta, np.abs(xi0).max(axis=1) <= XI_CLOSED


@pytest.mark.parametrize("name", CLOSED)
def test_twin_recovers_the_offset_and_the_reference_point(name):
    """x_elem(xi0) + delta nu has its foot at xi0 and lies |delta| away, on curves (nu any unit vector of the normal
    plane) and on surfaces alike."""
    geom, el, xi0, delta, sel = _closed_subset(name)
    tw = case_twin(name)
    assert sel.sum() >= (1 if len(el) < 8 else len(el) // 2)
    derr = np.abs(tw.distances - np.abs(delta))[sel].max()
    xerr = np.abs(tw.xi - xi0)[sel].max()
    print(f"{name}: |distance - |delta|| <= {derr:.1e}, |xi - xi0| <= {xerr:.1e}")
    assert np.array_equal(tw.elements[sel], el[sel])
    assert derr <= 1e-12 and xerr <= 1e-12
    if name in CURVES:
        assert tw.xi.shape[1] == 1


@pytest.mark.parametrize("name", CLOSED)
def test_twin_reproduces_affine_fields(name):
    """z = a.x + b on the nodes: an isoparametric element reproduces it (sum phi_i = 1), so the value is a.foot + b and
    the tangential gradient the projection J (J^T J)^-1 J^T a of a onto the tangent space."""
    geom, el, xi0, delta, sel = _closed_subset(name)
    tw = case_twin(name)
    z, a, b = affine_field(geom)
    vals, grads = tw.evaluate(z, gradient=True)
    _, J = element_frame(geom, tw.elements, tw.xi)
    A = np.einsum("bad,baf->bdf", J, J)
    want = np.einsum("bad,bd->ba", J, np.linalg.solve(A, np.einsum("bad,a->bd", J, a)[..., None])[..., 0])
    verr = np.abs(vals[:, 0] - (tw.points @ a + b)).max()
    gerr = np.abs(grads[:, 0] - want).max()
    print(f"{name}: value error {verr:.1e}, gradient error {gerr:.1e}")
    assert verr <= 1e-12 and gerr <= 1e-12
    if name.startswith("flat"):
        n = np.array([0.0, 0.0, 1.0])
        assert np.abs(grads[:, 0] - (a - (a @ n) * n)).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# the input condition of the GPU cases
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_cases_meet_the_input_condition_on_the_twin(name):
    tw = case_twin(name)
    close = int((tw.margin < 1e-9).sum())
    print(f"{name}: smallest margin {tw.margin.min():.2e}, {close} below 1e-9, at most {tw.all_iterations.max()} iterations")
    assert tw.all_converged.all()
    assert tw.all_iterations.max() <= DEVICE_MAXIT                   # the device stops at 64
    assert close <= 0.05 * tw.margin.size
    assert (tw.elements >= 0).all() and tw.converged.all()


@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_special_points_converge_on_the_twin(name):
    geom, P, md, tw = special(name)
    assert tw.all_converged.all() and tw.all_iterations.max() <= DEVICE_MAXIT
    if name.startswith(("without", "nonfinite")):
        assert (tw.elements == -1).all() and np.isnan(tw.distances).all() and np.isnan(tw.xi).all()
    else:
        assert (tw.elements >= 0).all()
    if name.startswith(("arc", "vertex")):
        assert (np.abs(tw.xi) == 1.0).all()
    if name.startswith("flat_outside"):
        assert (np.abs(tw.xi) == 1.0).any(axis=1).sum() >= 2
    if name.startswith("vertex"):                                     # the vertex is shared: the lower element reports it
        assert (tw.margin < 1e-12).all()
        V = geom.x[0]
        assert np.abs(tw.points - V).max() <= 1e-15
