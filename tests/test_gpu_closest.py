"""closest_point / ClosestPointLocator on the device against the NumPy twin (tests/closest_twin.py), whose own checks
against closed forms run without a GPU in tests/test_closest.py.  The cases are those of tests/closest_cases.py.

Bounds.  The twin and the device run the same iteration in double precision with differently associated sums, so both
stop within one stopping tolerance of the same minimiser: xi agrees within
tol_xi = max(1e-10, 4 ROUND_FACTOR EPS max|x| |(J^T J)^-1 J^T|_inf) per point, a value within tol_xi x dudxi (the change of
the value per unit change of xi) + 1e-12 max|z| (the rounding of the sum itself), distances and feet within 1e-10 x the
diagonal of the mesh's box, the project's parity standard."""
import numpy as np
import pytest

import mgb_amd as m
from closest_cases import (CASES, CLAMPED, DISTANCE_ONLY, NO_FOOT, SPECIAL, XI_CLOSED, affine_field, case, case_twin,
                           element_frame, mesh, mesh_diagonal, smooth_fields, special)
from test_closest import CLOSED
from test_manifold_post import flat_pair

pytestmark = pytest.mark.gpu


def _locate(geom, pts, md=None):
    with m.ClosestPointLocator(geom, pts, max_distance=md) as cp:
        return cp.elements, cp.xi, cp.points, cp.distances, cp.converged, cp.max_distance


@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_the_twin(name):
    geom, pts = case(name)[:2]
    tw = case_twin(name)
    Z = smooth_fields(geom)
    with m.ClosestPointLocator(geom, pts) as cp:
        elem, xi, feet, dist, conv = cp.elements, cp.xi, cp.points, cp.distances, cp.converged
        vals, grads = cp.evaluate(Z, gradient=True)
        assert cp.max_distance == tw.max_distance
    M = pts.shape[0]
    assert elem.dtype == np.int32 and elem.shape == (M,) and conv.dtype == bool and conv.all()
    clear = tw.margin >= 1e-9
    assert np.array_equal(elem[clear], tw.elements[clear])
    for q in np.nonzero(~clear)[0]:
        assert elem[q] in tw.tied(q)
    ar = np.arange(M)
    txi, tfeet, tdist = tw.all_xi[ar, elem], tw.all_points[ar, elem], tw.all_distances[ar, elem]
    tol = tw.tol_xi(elem, txi)
    diag = mesh_diagonal(geom)
    exi = np.abs(xi - txi).max(axis=1)
    tv, tg = tw.evaluate(Z, elem, txi, gradient=True)
    vtol = tol[:, None] * tw.dudxi(Z, elem, txi) + 1e-12 * np.abs(Z).max(axis=0)[None, :]
    ev = np.abs(vals - tv)
    print(f"{name}: xi {exi.max():.2e} (tol {tol.min():.2e}..{tol.max():.2e}), distance {np.abs(dist - tdist).max() / diag:.2e} "
          f"diag, foot {np.abs(feet - tfeet).max() / diag:.2e} diag, value/tol {np.max(ev / vtol):.2e}, "
          f"gradient {np.abs(grads - tg).max():.2e} (max {np.abs(tg).max():.2e})")
    assert (exi <= tol).all()
    assert (ev <= vtol).all()
    assert np.abs(dist - tdist).max() <= 1e-10 * diag and np.abs(feet - tfeet).max() <= 1e-10 * diag


@pytest.mark.parametrize("name", CLOSED)
def test_closed_forms_on_the_device(name):
    geom, pts, el, xi0, delta, nu = case(name)
    sel = np.abs(xi0).max(axis=1) <= XI_CLOSED
    z, a, b = affine_field(geom)
    with m.ClosestPointLocator(geom, pts) as cp:
        elem, xi, feet, dist = cp.elements, cp.xi, cp.points, cp.distances
        vals, grads = cp.evaluate(z, gradient=True)
    assert np.array_equal(elem[sel], el[sel])
    derr, xerr = np.abs(dist - np.abs(delta))[sel].max(), np.abs(xi - xi0)[sel].max()
    _, J = element_frame(geom, elem, xi)
    A = np.einsum("bad,baf->bdf", J, J)
    want = np.einsum("bad,bd->ba", J, np.linalg.solve(A, np.einsum("bad,a->bd", J, a)[..., None])[..., 0])
    verr, gerr = np.abs(vals - (feet @ a + b)).max(), np.abs(grads - want).max()
    print(f"{name}: distance {derr:.1e}, xi {xerr:.1e}, value {verr:.1e}, gradient {gerr:.1e}")
    assert derr <= 1e-12 and xerr <= 1e-12 and verr <= 1e-12 and gerr <= 1e-12
    if name.startswith("flat"):
        n = np.array([0.0, 0.0, 1.0])
        assert np.abs(grads - (a - (a @ n) * n)).max() <= 1e-12


@pytest.mark.parametrize("k", [1, 2])
def test_flat_surface_agrees_with_interpolate_on_the_flat_twin_mesh(k):
    g2, g3 = flat_pair(k)
    rng = np.random.default_rng(5)
    lo, hi = g2.xflat.min(axis=0), g2.xflat.max(axis=0)
    pts2 = rng.uniform(lo + 0.02, hi - 0.02, size=(257, 2))
    Z = smooth_fields(g2)
    ref, el2 = m.interpolate(g2, Z, pts2, return_element=True)
    keep = el2 >= 0                                                    # the curved k = 2 square is not the box of its nodes
    assert keep.sum() >= 200
    pts3 = np.concatenate([pts2, np.zeros((257, 1))], axis=1)
    vals, el3, dist = m.closest_point(g3, Z, pts3, return_element=True, return_distance=True)
    err = (np.abs(vals - ref)[keep] / np.abs(Z).max(axis=0)[None, :]).max()
    print(f"k = {k}: values against interpolate {err:.2e} max|z| per column, distances {np.abs(dist[keep]).max():.2e}")
    assert err <= 1e-10
    assert np.abs(dist[keep]).max() <= 1e-10 * mesh_diagonal(g3)


@pytest.mark.parametrize("name", sorted(SPECIAL))
def test_special_points(name):
    geom, P, md, tw = special(name)
    n = geom.x.shape[0] * geom.x.shape[1]
    first = _locate(geom, P, md)
    second = _locate(geom, P, md)
    for a, b in zip(first, second):                                     # bitwise the same on a second run
        assert np.array_equal(a, b, equal_nan=True)
    elem, xi, feet, dist, conv, _ = first
    diag = mesh_diagonal(geom)
    if name in NO_FOOT:
        assert (elem == -1).all() and not conv.any()
        assert np.isnan(xi).all() and np.isnan(feet).all() and np.isnan(dist).all()
        v, g = m.closest_point(geom, np.ones((n, 2)), P, max_distance=md, gradient=True)
        assert np.isnan(v).all() and np.isnan(g).all() and g.shape == v.shape + (geom.x.shape[2],)
        return
    assert (elem >= 0).all()
    print(f"{name}: distance error {np.abs(dist - tw.distances).max() / diag:.2e} diag")
    assert np.abs(dist - tw.distances).max() <= 1e-10 * diag
    if name in DISTANCE_ONLY and not name.startswith("vertex"):
        return
    assert np.array_equal(elem, tw.elements)                          # a shared vertex reports the lower element, as the twin
    assert np.array_equal(np.abs(xi) == 1.0, np.abs(tw.xi) == 1.0)     # a clamped axis is at exactly +-1
    assert np.abs(xi - tw.xi).max() <= tw.tol_xi().max()
    if name in CLAMPED:
        assert (np.abs(xi) == 1.0).any()


def test_bitwise_identities():
    geom, pts = case("sphere_m2_k2")[:2]
    pts = np.concatenate([pts, [[np.nan, 0.0, 0.0], [9.0, 9.0, 9.0]]])
    Z = smooth_fields(geom)
    with m.ClosestPointLocator(geom, pts) as cp:
        vals = cp.evaluate(Z)
        v2, grads = cp.evaluate(Z, gradient=True)
        assert np.array_equal(vals, v2, equal_nan=True)                  # the values do not depend on the gradient
        assert np.isnan(vals[-2:]).all() and np.isnan(grads[-2:]).all() and np.isfinite(vals[:-2]).all()
        assert vals.shape == (259, 3) and grads.shape == (259, 3, 3)
        for c in range(3):                                               # a column is its one-column call
            one, gone = cp.evaluate(Z[:, c], gradient=True)
            assert one.shape == (259,) and gone.shape == (259, 3)
            assert np.array_equal(one, vals[:, c], equal_nan=True) and np.array_equal(gone, grads[:, c], equal_nan=True)
            assert np.array_equal(cp.evaluate(Z[:, c:c + 1])[:, 0], vals[:, c], equal_nan=True)
        elem, dist = cp.elements, cp.distances
    with pytest.raises(ValueError, match="^ClosestPointLocator: the locator is closed$"):
        cp.evaluate(Z)
    with pytest.raises(ValueError, match="^ClosestPointLocator: the locator is closed$"):
        cp.xi
    v, g, el, di = m.closest_point(geom, Z, pts, gradient=True, return_element=True, return_distance=True)
    assert np.array_equal(v, vals, equal_nan=True) and np.array_equal(g, grads, equal_nan=True)
    assert np.array_equal(el, elem) and np.array_equal(di, dist, equal_nan=True)
    assert np.array_equal(m.closest_point(geom, Z[:, 0], pts), vals[:, 0], equal_nan=True)
    one = m.closest_point(geom, Z[:, 0], pts[3])                          # one point (e,): scalars
    assert isinstance(one, float) and one == vals[3, 0]
    with m.ClosestPointLocator(geom, pts[3]) as cp1:
        assert cp1.elements == elem[3] and cp1.xi.shape == (2,) and cp1.points.shape == (3,) and cp1.distances == dist[3]
        assert cp1.converged is True


def test_max_distance_cuts_off_and_widens():
    geom = mesh("circle3_k2")
    _, pts, el, xi0, delta, nu = case("circle3_k2")
    srt = np.sort(np.abs(delta))
    cut = float(0.5 * (srt[128] + srt[129]))                            # between two of the 257 distances
    with m.ClosestPointLocator(geom, pts, max_distance=cut) as cp:
        elem, dist = cp.elements, cp.distances
    tw = case_twin("circle3_k2")
    near = tw.distances <= cut
    assert np.array_equal(elem >= 0, near) and 0 < near.sum() < near.size
    assert np.array_equal(elem[near], tw.elements[near]) and (dist[near] <= cut).all()
    with m.ClosestPointLocator(geom, pts, max_distance=0.0) as cp0:         # nothing is exactly on the curve
        assert (cp0.elements == -1).all()
