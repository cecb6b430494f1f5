"""PointLocator on the device, pinned to `interpolate()` bit for bit.

`PointLocator.evaluate` runs the locate and the evaluate half of the fused query kernels in two launches, with the
reference coordinates the fused kernel evaluates at stored in between; the file is compiled without FMA contraction, so
both paths run the same IEEE operations on the same numbers.  Equality is therefore exact (`np.array_equal` with NaN
positions equal): no tolerance appears below except in the anchor of section 3, which does not go through
`interpolate()` and uses the bounds `tests/test_gpu_interpolate.py` and `tests/test_gpu_interpolate_gradient.py` use for
the same polynomial checks.
"""
import zlib

import numpy as np
import pytest

import mgb_amd as m
from test_gpu_interpolate import REPRO_RTOL, _interior, _relerr, _repro_geom
from test_gpu_interpolate_gradient import DEVICE_FACTOR, EPS, TWIN_CAP, _as2d, _poly_ld, _ratios, host_gradients

pytestmark = pytest.mark.gpu


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _fem1d_unsorted(k):
    """fem1d with the elements in a shuffled order (the device then scans instead of bisecting)."""
    g = m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 4), k=k), 3)
    perm = np.random.default_rng(5).permutation(g.x.shape[1])
    return m.fem1d(k=k, K=g.x[:, perm, :].copy())


CASES = {
    "fem1d_k1": lambda: m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 4), k=1), 4),
    "fem1d_k3": lambda: m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 4), k=3), 4),
    "fem1d_k1_unsorted": lambda: _fem1d_unsorted(1),
    "fem1d_k3_unsorted": lambda: _fem1d_unsorted(3),
    "fem2d_k1": lambda: m.subdivide(m.fem2d(k=1), 3),
    "fem2d_k2": lambda: m.subdivide(m.fem2d(k=2), 3),
    "fem2d_k4": lambda: m.subdivide(m.fem2d(k=4), 2),
    "fem2d_k2_curved": lambda: m.fem2d(k=2, K=_curve(m.subdivide(m.fem2d(k=2), 3).x)),
    "fem3d_k1": lambda: m.subdivide(m.fem3d(k=1), 2),
    "fem3d_k2": lambda: m.subdivide(m.fem3d(k=2), 2),
    "fem2d_P1": lambda: m.subdivide(m.fem2d_P1(), 4),
    "fem2d_P2": lambda: m.subdivide(m.fem2d_P2(), 4),
    "fem2d_P2_nobubble": lambda: m.subdivide(m.fem2d_P2(bubble=False), 4),
    "spectral1d": lambda: m.spectral1d(n=12),
    "spectral2d": lambda: m.spectral2d(n=8),
}


def _curve(X):
    """A smooth, non-polynomial map of [-1, 1]^2 applied to every node: the Q2 elements get curved edges."""
    Y = X.copy()
    Y[..., 0] += 0.08 * np.sin(np.pi * X[..., 1])
    Y[..., 1] += 0.06 * np.sin(np.pi * X[..., 0]) * X[..., 1]
    return Y


def _mixed_points(geom, rng, M=4000):
    """Random interior points, mesh nodes, points on shared faces (midpoints of node pairs of an element), points
    outside, NaN and +-Inf; 1-D: a vector, else (M, d)."""
    d = geom.x.shape[2]
    X = geom.xflat
    lo, hi = X.min(axis=0), X.max(axis=0)
    parts = [rng.uniform(lo, hi, size=(M, d)),
             X[rng.integers(0, X.shape[0], size=M // 4)],
             X.copy() if X.shape[0] <= M else X[:M]]
    p = geom.x.shape[0]
    e = rng.integers(0, geom.x.shape[1], size=M // 4)
    i, j = rng.integers(0, p, size=M // 4), rng.integers(0, p, size=M // 4)
    parts.append(0.5 * (geom.x[i, e, :] + geom.x[j, e, :]))
    parts.append(rng.uniform(lo - 1.0, hi + 1.0, size=(M // 8, d)))            # many of them outside
    special = np.array([np.nan, np.inf, -np.inf, 0.0])
    parts.append(special[rng.integers(0, 4, size=(24, d))])
    parts.append(np.stack([lo, hi, lo - 1e-13, hi + 1e-13]))
    pts = np.concatenate(parts, axis=0)
    pts = pts[rng.permutation(pts.shape[0])]
    return pts[:, 0] if d == 1 else pts


@pytest.fixture(params=sorted(CASES), scope="module")
def case(request):
    geom = CASES[request.param]()
    rng = np.random.default_rng(zlib.crc32(request.param.encode()))
    return request.param, geom, rng, _mixed_points(geom, rng)


# ---------------------------------------------------------------------------------------------------------------------
# 1. bitwise equality with interpolate(): values, gradients, elements
# ---------------------------------------------------------------------------------------------------------------------

def test_values_gradients_and_elements_are_bitwise_interpolates(case):
    name, geom, rng, pts = case
    n = geom.xflat.shape[0]
    z = rng.standard_normal(n)
    v0, e0 = m.interpolate(geom, z, pts, return_element=True)
    v1, g1, e1 = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    with m.PointLocator(geom, pts) as loc:
        assert loc.n_points == np.asarray(pts).shape[0] and not loc.closed
        assert _eq(loc.evaluate(z), v0), name
        v, g = loc.evaluate(z, gradient=True)
        assert _eq(v, v1) and _eq(g, g1), name
        assert _eq(loc.elements, e0) and _eq(loc.elements, e1), name
        assert loc.elements.dtype == np.int32
    if not name.startswith("spectral"):
        assert np.isnan(v0).any(), "the point set is meant to hold points without a value"
    if not name.startswith(("spectral", "fem1d")):
        assert (e0 < 0).any() and (e0 >= 0).sum() > e0.size // 2


def test_one_point_and_scalar_shapes(case):
    name, geom, rng, pts = case
    z = rng.standard_normal((geom.xflat.shape[0], 2))
    d = geom.x.shape[2]
    one = 0.25 if d == 1 else np.full(d, 0.25)
    with m.PointLocator(geom, one) as loc:
        for zz in (z, z[:, 1]):
            v0, g0, e0 = m.interpolate(geom, zz, one, gradient=True, return_element=True)
            v, g = loc.evaluate(zz, gradient=True)
            assert type(v) is type(v0) and type(g) is type(g0) and _eq(v, v0) and _eq(g, g0)
            assert type(loc.elements) is type(e0) and loc.elements == e0
            assert _eq(loc.evaluate(zz), m.interpolate(geom, zz, one))


# ---------------------------------------------------------------------------------------------------------------------
# 2. reuse: one locator, several z in a row
# ---------------------------------------------------------------------------------------------------------------------

def test_one_locator_many_z(case):
    name, geom, rng, pts = case
    n = geom.xflat.shape[0]
    z1, Z5, z3 = rng.standard_normal(n), rng.standard_normal((n, 5)), rng.standard_normal(n)
    with m.PointLocator(geom, pts) as loc:
        a = loc.evaluate(z1)
        B, GB = loc.evaluate(Z5, gradient=True)
        c, gc = loc.evaluate(z3, gradient=True)
        a2 = loc.evaluate(z1)
        for j in range(5):
            vj, gj = loc.evaluate(Z5[:, j], gradient=True)
            assert _eq(B[..., j], vj) and _eq(GB[:, j], gj), (name, j)
    assert _eq(a, m.interpolate(geom, z1, pts)) and _eq(a2, a)
    B0, GB0 = m.interpolate(geom, Z5, pts, gradient=True)
    assert _eq(B, B0) and _eq(GB, GB0)
    c0, gc0 = m.interpolate(geom, z3, pts, gradient=True)
    assert _eq(c, c0) and _eq(gc, gc0)


def test_locator_holds_copies_of_points_and_nodes():
    geom = m.subdivide(m.fem2d(k=2), 2)
    rng = np.random.default_rng(11)
    pts = _interior(rng, 500, 2)
    z = rng.standard_normal(geom.xflat.shape[0])
    want = m.interpolate(geom, z, pts, gradient=True)
    keep_pts, keep_x = pts.copy(), geom.x.copy()
    with m.PointLocator(geom, pts) as loc:
        pts[:] = 0.0
        geom.x[:] = 7.0
        v, g = loc.evaluate(z, gradient=True)
    pts[:], geom.x[:] = keep_pts, keep_x
    assert _eq(v, want[0]) and _eq(g, want[1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. an anchor that does not go through interpolate(): polynomials of the element space
# ---------------------------------------------------------------------------------------------------------------------

ANCHOR = [("fem1d", 3), ("fem2d", 2), ("fem3d", 2), ("fem2d_P1", 1), ("fem2d_P2", 2), ("fem2d_P2_nobubble", 2)]


@pytest.mark.parametrize("name,k", ANCHOR)
def test_locator_reproduces_polynomials_and_their_gradients(name, k):
    rng = np.random.default_rng(zlib.crc32(f"locator{name}{k}".encode()))
    geom, d, deg = _repro_geom(name, k)
    total = name.startswith("fem2d_P")
    f = _poly_ld(rng, d, deg, total=total)
    z = f(geom.xflat).astype(np.float64)
    pts = _interior(rng, 20_000, d)
    with m.PointLocator(geom, pts[:, 0] if d == 1 else pts) as loc:
        vals, grads = loc.evaluate(z, gradient=True)
        elem = loc.elements
    assert np.all(elem >= 0) and np.all(np.isfinite(vals))
    err = _relerr(vals, f(pts).astype(np.float64))
    print(f"locator reproduction {name} k={k}: max rel err {err:.3e}")
    assert err <= REPRO_RTOL, err
    g, g64, S = host_gradients(geom, z, elem, pts)
    exact = np.stack([f(pts, da=a) for a in range(d)], axis=1)
    r_dev, _ = _ratios(_as2d(grads), exact, g64, S)
    _, r_twin_oracle = _ratios(_as2d(grads), g, g64, S)
    line = f"locator gradient polynomial {name} k={k}: device {r_dev / EPS:.2f} eps, twin {r_twin_oracle / EPS:.2f} eps"
    print(line)
    assert r_twin_oracle <= TWIN_CAP, line
    assert r_dev <= DEVICE_FACTOR * r_twin_oracle + EPS / 2, line


# ---------------------------------------------------------------------------------------------------------------------
# 4. the callers the locator is for
# ---------------------------------------------------------------------------------------------------------------------

def test_parabolic_trajectory_through_one_locator():
    mg = m.amg(m.subdivide(m.fem2d_P2(), 3))
    sol = m.parabolic_solve(mg, h=0.25, t1=0.5, p=1.5, f1=lambda t, x: 0.5 + 0.25 * t * x[0])
    assert len(sol.u) == 3
    g = np.linspace(-1, 1, 41)
    raster = np.stack(np.meshgrid(g, g, indexing="ij"), axis=-1).reshape(-1, 2)
    with m.PointLocator(sol.geometry, raster) as loc:
        frames = [loc.evaluate(u[:, 0]) for u in sol.u]
    for u, frame in zip(sol.u, frames):
        assert _eq(frame, m.interpolate(sol.geometry, u[:, 0], raster))
        assert np.all(np.isfinite(frame))
    assert not _eq(frames[0], frames[-1])


def test_two_locators_alive_at_once():
    rng = np.random.default_rng(21)
    ga, gb = m.subdivide(m.fem2d_P2(), 3), m.subdivide(m.fem3d(k=2), 2)
    pa, pb = _interior(rng, 3000, 2), _interior(rng, 2000, 3)
    za, zb = rng.standard_normal(ga.xflat.shape[0]), rng.standard_normal(gb.xflat.shape[0])
    with m.PointLocator(ga, pa) as la, m.PointLocator(gb, pb) as lb:
        vb = lb.evaluate(zb)
        va = la.evaluate(za)
        vb2, gb2 = lb.evaluate(zb, gradient=True)
        ea, eb = la.elements, lb.elements
    assert _eq(va, m.interpolate(ga, za, pa)) and _eq(vb, m.interpolate(gb, zb, pb)) and _eq(vb2, vb)
    assert _eq(gb2, m.interpolate(gb, zb, pb, gradient=True)[1])
    assert _eq(ea, m.interpolate(ga, za, pa, return_element=True)[1])
    assert _eq(eb, m.interpolate(gb, zb, pb, return_element=True)[1])


def test_two_million_points_on_p2():
    geom = m.subdivide(m.fem2d_P2(), 7)
    rng = np.random.default_rng(31)
    pts = rng.uniform(-1, 1, (2 * 2 ** 20, 2))
    a = rng.standard_normal(6)
    X = geom.xflat
    z = a[0] + a[1] * X[:, 0] + a[2] * X[:, 1] + a[3] * X[:, 0] ** 2 + a[4] * X[:, 0] * X[:, 1] + a[5] * X[:, 1] ** 2
    v0, g0, e0 = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    with m.PointLocator(geom, pts) as loc:
        v, g = loc.evaluate(z, gradient=True)
        assert _eq(v, v0) and _eq(g, g0) and _eq(loc.elements, e0)
        assert _eq(loc.evaluate(z), v0)
    assert np.all(e0 >= 0)
