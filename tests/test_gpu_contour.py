"""isocontour() on the device against the NumPy twin (tests/contour_twin.py).

The twin and the kernel follow the same four steps, so the combinatorial part of the result (`S`, `level`, `element`) must
agree exactly once no lattice value is so close to a level that two summation orders could classify it differently:
every case first asserts, on the twin alone, that the smallest |lattice value - level| exceeds 1024 eps max|z| (the cases
and that check live in tests/test_contour.py, where they also run without a GPU).

`points` and `carried` are compared against a per-vertex bound.  The lattice values on both sides are sums of p
products, so they carry an error of about p eps max|z|; the crossing parameter t = (c - v_a) / (v_b - v_a) amplifies
it by 1 / |v_b - v_a|, and the vertex moves by that times |x_b - x_a|.  The bound is therefore

    DEVICE_FACTOR p eps max|z| / |v_b - v_a| * |x_b - x_a|  +  8 eps max|x|

(and the same with the carried field in place of x), with DEVICE_FACTOR = 16 imported from
tests/test_gpu_interpolate_gradient.py, the allowance that file gives a device sum against a host sum of another order.
"""
import ctypes as C

import numpy as np
import pytest

import mgb_amd as m
from contour_twin import isocontour_twin
from helpers import record_observation
from test_contour import (EPS, GPU_CASES, LEVELS1, LEVELS5, PLANES, check_linear, input_margin_ok, smooth)
from test_gpu_interpolate_gradient import DEVICE_FACTOR

pytestmark = pytest.mark.gpu


def _eq(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(c0, c1):
    return _eq(c0.points, c1.points) and _eq(c0.level, c1.level) and _eq(c0.element, c1.element) and _eq(c0.carried, c1.carried)


@pytest.fixture(params=sorted(GPU_CASES), scope="module")
def case(request):
    make, other = GPU_CASES[request.param]
    geom = make()
    z, carry = smooth(geom.xflat)
    return request.param, geom, other, z, carry


# ---------------------------------------------------------------------------------------------------------------------
# 1. comparison with the twin
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_carry", [False, True], ids=["plain", "carry"])
@pytest.mark.parametrize("nlev", [1, 5])
@pytest.mark.parametrize("which", ["default", "other"])
def test_matches_the_twin(case, which, nlev, with_carry):
    name, geom, other, z, carry = case
    refine = None if which == "default" else other
    levels = LEVELS1 if nlev == 1 else LEVELS5
    cr = carry if with_carry else None
    t = isocontour_twin(geom, z, levels, refine=refine, carry=cr)
    assert input_margin_ok(t, z), (name, refine, t.margin)
    c = m.isocontour(geom, z, levels, refine=refine, carry=cr)
    d, p = geom.x.shape[2], geom.x.shape[0]
    assert c.points.shape == (c.level.size, d, d) and c.points.dtype == np.float64
    assert c.level.dtype == np.int32 and c.element.dtype == np.int32
    assert c.level.size == t.level.size and c.level.size > 0, (name, c.level.size, t.level.size)
    assert np.array_equal(c.level, t.level) and np.array_equal(c.element, t.element)
    amp = DEVICE_FACTOR * p * EPS * np.abs(z).max() / t.dv                      # (S, d): the error of t
    bound = amp * t.dx + 8 * EPS * np.abs(geom.xflat).max()
    err = np.abs(c.points - t.points).max(axis=2)
    ratio = float((err / bound).max())
    line = f"isocontour vs twin {name} refine={refine} nlev={nlev}: S = {c.level.size}, points error / bound {ratio:.3e}"
    if with_carry:
        assert c.carried.shape == (c.level.size, d, 2)
        cbound = amp[..., None] * t.dc + 8 * EPS * np.abs(carry).max()
        cratio = float((np.abs(c.carried - t.carried) / cbound).max())
        line += f", carried error / bound {cratio:.3e}"
    else:
        assert c.carried is None
        cratio = 0.0
    print(line)
    record_observation(line)
    assert ratio <= 1.0 and cratio <= 1.0, line
    assert np.allclose(c.measure(), t.measure(), rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. determinism
# ---------------------------------------------------------------------------------------------------------------------

def test_two_calls_are_bitwise_equal_and_ordered(case):
    name, geom, other, z, carry = case
    for refine in (None, other):
        a = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry)
        b = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry)
        assert _same(a, b), name
        assert a.level.size > 0 and np.all(np.diff(a.element) >= 0)
        assert a.level.min() >= 0 and a.level.max() <= 4
        for j in range(2):
            one = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry[:, j])
            assert _eq(one.carried[..., 0], a.carried[..., j]) and _eq(one.points, a.points), (name, j)
        plain = m.isocontour(geom, z, LEVELS5, refine=refine)
        assert _eq(plain.points, a.points) and _eq(plain.level, a.level) and _eq(plain.element, a.element)


def test_duplicate_levels_are_separate_levels(case):
    name, geom, other, z, carry = case
    c1 = m.isocontour(geom, z, LEVELS1)
    c2 = m.isocontour(geom, z, [LEVELS1[0], LEVELS1[0]])
    assert c2.level.size == 2 * c1.level.size
    assert _eq(c2.points[c2.level == 0], c1.points) and _eq(c2.points[c2.level == 1], c1.points)
    assert _eq(c2.element[c2.level == 1], c1.element)
    scalar = m.isocontour(geom, z, float(LEVELS1[0]))
    assert _same(scalar, c1)


def test_vertices_inside_an_element_are_shared_bit_for_bit():
    geom = m.subdivide(m.fem3d(k=2), 2)
    z, _ = smooth(geom.xflat)
    c = m.isocontour(geom, z, LEVELS1, refine=4)
    P = c.points[c.element == 0].reshape(-1, 3)
    _, counts = np.unique(P, axis=0, return_counts=True)
    assert counts.max() >= 3 and (counts >= 2).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------
# 3. slices and linear functions
# ---------------------------------------------------------------------------------------------------------------------

def test_slice_of_a_linear_function():
    geom = m.subdivide(m.fem3d(k=1), 3)
    X = geom.xflat
    a, b, _ = PLANES[1]
    a = np.asarray(a)
    z = X @ a + b
    cut = 0.3
    c = m.isocontour(geom, X[:, 0].copy(), [cut], carry=z)
    assert c.level.size > 0
    print(f"slice: S = {c.level.size}, |x - c| max {np.abs(c.points[..., 0] - cut).max() / EPS:.2f} eps, "
          f"carried residual {np.abs(c.carried[..., 0] - (c.points @ a + b)).max() / EPS:.2f} eps")
    assert np.abs(c.points[..., 0] - cut).max() <= 8 * EPS
    assert np.abs(c.carried[..., 0] - (c.points @ a + b)).max() <= 64 * EPS * np.abs(z).max()
    # the slice is the whole cross-section of the cube
    assert abs(c.measure()[0] - 4.0) <= c.level.size * 8 * EPS * 2 * np.sqrt(3)


def test_device_cuts_linear_functions_exactly():
    geom = m.subdivide(m.fem3d(k=1), 3)
    for a, b, cc in PLANES:
        check_linear("fem3d_Q1 device", geom, m.isocontour(geom, geom.xflat @ np.asarray(a) + b, [cc]), a, b, cc)


def test_circle_and_sphere_converge_on_the_device():
    g2 = m.subdivide(m.fem2d(k=2), 3)
    z2 = (g2.xflat ** 2).sum(axis=1)
    e2 = [abs(m.isocontour(g2, z2, 0.37, refine=r).measure()[0] - 2 * np.pi * np.sqrt(0.37)) for r in (2, 4, 8)]
    g3 = m.subdivide(m.fem3d(k=2), 2)
    z3 = (g3.xflat ** 2).sum(axis=1)
    e3 = [abs(m.isocontour(g3, z3, 0.37, refine=r).measure()[0] - 4 * np.pi * 0.37) for r in (2, 4)]
    print("device circle errors", e2, "sphere errors", e3)
    assert e2[1] <= e2[0] / 2 and e2[2] <= e2[1] / 2 and e3[1] <= e3[0] / 2


# ---------------------------------------------------------------------------------------------------------------------
# 4. non-finite values, levels outside the range, the largest lattices
# ---------------------------------------------------------------------------------------------------------------------

def test_nan_node_removes_only_the_simplices_that_touch_it(case):
    name, geom, other, z, carry = case
    p, N, d = geom.x.shape
    good = m.isocontour(geom, z, LEVELS5, carry=carry)
    e = int(good.element[good.element.size // 2])            # an element that is cut
    zb = z.copy()
    zb[e * p] = np.nan                                        # local node 0 of element e
    bad = m.isocontour(geom, zb, LEVELS5, carry=carry)
    tb = isocontour_twin(geom, zb, LEVELS5, carry=carry)
    assert np.array_equal(bad.level, tb.level) and np.array_equal(bad.element, tb.element)
    assert (bad.element == e).sum() < (good.element == e).sum(), name
    keep_g, keep_b = good.element != e, bad.element != e
    assert _eq(good.points[keep_g], bad.points[keep_b]) and _eq(good.level[keep_g], bad.level[keep_b])
    assert _eq(good.element[keep_g], bad.element[keep_b]) and _eq(good.carried[keep_g], bad.carried[keep_b])
    assert np.all(np.isfinite(bad.points)) and np.all(np.isfinite(bad.carried))


def test_level_outside_the_range_gives_nothing(case):
    name, geom, other, z, carry = case
    d = geom.x.shape[2]
    for lev in (z.max() + 1.0, z.min() - 1.0, [z.max() + 1.0, z.max() + 2.0]):
        c = m.isocontour(geom, z, lev, carry=carry)
        assert c.points.shape == (0, d, d) and c.level.shape == (0,) and c.element.shape == (0,)
        assert c.carried.shape == (0, d, 2)


@pytest.mark.parametrize("name,make,refine", [
    ("fem2d_k8", lambda: m.subdivide(m.fem2d(k=8), 2), 16),
    ("fem3d_k8", lambda: m.fem3d(k=8), 8),
    ("fem3d_k2", lambda: m.subdivide(m.fem3d(k=2), 2), 8),
    ("fem2d_P2", lambda: m.subdivide(m.fem2d_P2(), 2), 16),
    ("fem2d_P1", lambda: m.subdivide(m.fem2d_P1(), 2), 16),
])
def test_largest_lattices_and_four_carried_fields(name, make, refine):
    geom = make()
    z, carry = smooth(geom.xflat)
    carry4 = np.concatenate([carry, geom.xflat[:, :1], z[:, None] ** 2], axis=1)
    t = isocontour_twin(geom, z, LEVELS5, refine=refine, carry=carry4)
    assert input_margin_ok(t, z)
    c = m.isocontour(geom, z, LEVELS5, refine=refine, carry=carry4)
    assert np.array_equal(c.level, t.level) and np.array_equal(c.element, t.element)
    p = geom.x.shape[0]
    amp = DEVICE_FACTOR * p * EPS * np.abs(z).max() / t.dv
    ratio = float((np.abs(c.points - t.points).max(axis=2) / (amp * t.dx + 8 * EPS * np.abs(geom.xflat).max())).max())
    cbound = amp[..., None] * t.dc + 8 * EPS * np.abs(carry4).max()
    cratio = float((np.abs(c.carried - t.carried) / cbound).max())
    line = f"isocontour vs twin {name} refine={refine} (cap): S = {c.level.size}, points {ratio:.3e}, carried {cratio:.3e} of the bound"
    print(line)
    record_observation(line)
    assert ratio <= 1.0 and cratio <= 1.0, line


# ---------------------------------------------------------------------------------------------------------------------
# 5. the C ABI, driven directly
# ---------------------------------------------------------------------------------------------------------------------

def test_c_abi_three_calls():
    from mgb_amd import device, fem2d_p1
    from mgb_amd.device import HipContext, _ptr
    from mgb_amd.interpolate import P1
    geom = m.subdivide(m.fem2d_P1(), 3)
    p, N, d = geom.x.shape
    X = np.ascontiguousarray(geom.xflat, dtype=np.float64)
    z, carry = smooth(X)
    F = np.ascontiguousarray(np.concatenate([z[:, None], carry[:, :1]], axis=1))
    table = np.ascontiguousarray(fem2d_p1.basis_coefficient_table())
    lev = np.ascontiguousarray(LEVELS5)
    ctx = HipContext(0)
    lib = ctx.lib
    ip = C.POINTER(C.c_int32)
    try:
        assert lib.mgbhip_contour_destroy(None) == device.OK
        h, n = C.c_void_p(), C.c_int64(-1)

        def create(refine, nfield=2, nlev=5, family=P1):
            return lib.mgbhip_contour_create(ctx.handle, family, d, 1, p, N, _ptr(X), _ptr(table), nfield, _ptr(F), nlev,
                                             _ptr(lev), refine, C.byref(h), C.byref(n))
        for bad in (0, 17, -3):
            assert create(bad) == device.ERR_INVALID
            msg = lib.mgbhip_last_error().decode()
            assert msg and "refine" in msg, msg
        assert create(2, nfield=6) == device.ERR_INVALID and lib.mgbhip_last_error()
        assert create(2, nfield=0) == device.ERR_INVALID and lib.mgbhip_last_error()
        assert create(2, family=1) == device.ERR_INVALID and lib.mgbhip_last_error()      # fem1d has no level sets
        assert create(2, nlev=-1) == device.ERR_INVALID and lib.mgbhip_last_error()
        lev_bad = lev.copy()
        lev_bad[3] = np.nan
        assert lib.mgbhip_contour_create(ctx.handle, P1, d, 1, p, N, _ptr(X), _ptr(table), 2, _ptr(F), 5, _ptr(lev_bad),
                                         2, C.byref(h), C.byref(n)) == device.ERR_INVALID
        assert h.value is None and n.value == -1, "a refused call leaves its outputs alone"

        assert create(2, nlev=0) == device.OK and n.value == 0 and h.value
        assert lib.mgbhip_contour_fetch(h, None, None, None, None) == device.OK
        assert lib.mgbhip_contour_destroy(h) == device.OK

        h = C.c_void_p()
        assert create(2) == device.OK, lib.mgbhip_last_error()
        S = int(n.value)
        want = m.isocontour(geom, z, LEVELS5, refine=2, carry=carry[:, 0])
        assert S == want.level.size and S > 0
        pts, lvl, elm, car = np.empty((S, 2, 2)), np.empty(S, np.int32), np.empty(S, np.int32), np.empty((S, 2, 1))
        assert lib.mgbhip_contour_fetch(h, _ptr(pts), lvl.ctypes.data_as(ip), elm.ctypes.data_as(ip), _ptr(car)) == device.OK
        assert _eq(pts, want.points) and _eq(lvl, want.level) and _eq(elm, want.element) and _eq(car, want.carried)
        pts2 = np.empty((S, 2, 2))
        assert lib.mgbhip_contour_fetch(h, _ptr(pts2), lvl.ctypes.data_as(ip), elm.ctypes.data_as(ip), None) == device.OK
        assert _eq(pts2, pts)
        assert lib.mgbhip_contour_fetch(h, None, lvl.ctypes.data_as(ip), elm.ctypes.data_as(ip), None) == device.ERR_INVALID
        assert lib.mgbhip_contour_fetch(None, _ptr(pts), lvl.ctypes.data_as(ip), elm.ctypes.data_as(ip), None) == device.ERR_INVALID
        assert lib.mgbhip_contour_destroy(h) == device.OK
    finally:
        ctx.close()
