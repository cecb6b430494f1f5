"""Curved (isoparametric) fem2d_P2 on the device (-m gpu): interpolate, PointLocator, isocontour, tessellate, StreamTracer
and a solve on the two meshes of tests/curved_p2_cases.py, built with `fem2d_P2(..., curved=True)`.

Points are manufactured (made in a known element at a known barycentric pair by the forward map in np.longdouble), so
where a point lies is known without inverting anything.  Values and gradients follow the scheme of
tests/test_gpu_interpolate_gradient.py, sections 1-2: an np.longdouble oracle (Newton from the manufactured pair), a
float64 NumPy twin with the device's documented stopping rule, and the device may differ from the oracle by DEVICE_FACTOR
times the twin's largest ratio, measured at run time; the twin itself stays below TWIN_CAP.  The error scales are
S(q) = sum_i |grad_x phi_i(q)|_inf |z_i| for the gradient and sum_i |phi_i(q)| |z_i| + max|x| S(q) for the value (the
rounding of the sum plus the rounding of the point).
"""
import zlib

import numpy as np
import pytest

import mgb_amd as m
from contour_twin import isocontour_twin
from curved_p2_cases import EPS, LD, MESHES, forward, host_reference, manufactured, mesh_a, mesh_b, ratios
from helpers import assert_z_close, record_observation
from manifold_twin import tessellate_twin
from mgb_amd.streamlines import StreamTracer
from streamlines_twin import trace_twin
from test_contour import LEVELS5, input_margin_ok, smooth
from test_gpu_interpolate import REPRO_RTOL, _relerr
from test_gpu_interpolate_gradient import DEVICE_FACTOR, TWIN_CAP
from test_gpu_locator import _eq, _mixed_points
from test_gpu_streamlines import interpolated, same
from test_streamlines import GPU_MAX_STEPS, GPU_MIN_SPEED, GPU_STEP, gpu_seeds

pytestmark = pytest.mark.gpu

M_POINTS = 20_000


@pytest.fixture(scope="module", params=[(mesh, b) for mesh in sorted(MESHES) for b in (True, False)],
                ids=lambda p: f"{p[0]}-{'bubble' if p[1] else 'nobubble'}")
def case(request):
    """One mesh with its 20 000 manufactured points (every barycentric coordinate >= 0.02), read-only."""
    mesh, bubble = request.param
    geom = MESHES[mesh](bubble)
    rng = np.random.default_rng(zlib.crc32(f"curvedP2{mesh}{bubble}".encode()))
    elem, made, pts = manufactured(geom, rng, M_POINTS)
    for a in (elem, made, pts):
        a.setflags(write=False)
    return f"{mesh} bubble={bubble}", geom, rng, elem, made, pts


# ---------------------------------------------------------------------------------------------------------------------
# 1. located where made
# ---------------------------------------------------------------------------------------------------------------------

def test_points_are_located_where_they_were_made(case):
    name, geom, rng, elem, made, pts = case
    z = rng.standard_normal(geom.xflat.shape[0])
    vals, found = m.interpolate(geom, z, pts, return_element=True)
    wrong = np.flatnonzero(found != elem)
    print(f"curved fem2d_P2 located where made, mesh {name}: {wrong.size} of {pts.shape[0]} points in another element")
    assert wrong.size == 0, (name, wrong[:10], found[wrong[:10]], elem[wrong[:10]])
    assert np.all(np.isfinite(vals))


# ---------------------------------------------------------------------------------------------------------------------
# 2. values and gradients against the extended-precision oracle
# ---------------------------------------------------------------------------------------------------------------------

def test_values_and_gradients_against_extended_precision_oracle(case):
    name, geom, rng, elem, made, pts = case
    z = rng.standard_normal(geom.xflat.shape[0])
    v0 = m.interpolate(geom, z, pts)
    vals, grads, found = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(found, elem) and np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
    assert np.array_equal(v0, vals)                                            # the values of gradient=True are bitwise
    v, v64, Sv, g, g64, S = host_reference(geom, z, elem, pts, made)
    rv_dev, rv_twin = ratios(vals, v, v64, Sv)
    rg_dev, rg_twin = ratios(grads, g, g64, S)
    line = (f"curved fem2d_P2 oracle mesh {name}: values device {rv_dev / EPS:.2f} eps, twin {rv_twin / EPS:.2f} eps; "
            f"gradients device {rg_dev / EPS:.2f} eps, twin {rg_twin / EPS:.2f} eps (of their scales), allowed "
            f"{DEVICE_FACTOR:.0f} x twin")
    print(line)
    record_observation(line)
    assert rv_twin <= TWIN_CAP and rg_twin <= TWIN_CAP, line
    assert rv_dev <= DEVICE_FACTOR * rv_twin, line
    assert rg_dev <= DEVICE_FACTOR * rg_twin, line


# ---------------------------------------------------------------------------------------------------------------------
# 3. affine functions are in an isoparametric space
# ---------------------------------------------------------------------------------------------------------------------

def test_affine_functions_and_their_gradients_are_reproduced(case):
    name, geom, rng, elem, made, pts = case
    a, b, c = rng.standard_normal(3)
    X = geom.xflat.astype(LD)
    z = (LD(a) + LD(b) * X[:, 0] + LD(c) * X[:, 1]).astype(np.float64)           # rounded once from longdouble
    vals, grads, found = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(found, elem)
    exact = a + b * pts[:, 0] + c * pts[:, 1]
    rel = _relerr(vals, exact)
    _, _, _, g, g64, S = host_reference(geom, z, elem, pts, made)
    target = np.broadcast_to(np.array([b, c], dtype=LD), g.shape)
    r_dev, _ = ratios(grads, target, g64, S)                                   # against the analytic gradient
    _, r_twin = ratios(grads, g, g64, S)                                       # the twin against the oracle
    line = (f"curved fem2d_P2 affine mesh {name}: values rel err {rel:.2e}, gradients device {r_dev / EPS:.2f} eps, twin "
            f"{r_twin / EPS:.2f} eps")
    print(line)
    record_observation(line)
    assert rel <= REPRO_RTOL, line
    assert r_twin <= TWIN_CAP, line
    assert r_dev <= DEVICE_FACTOR * r_twin + EPS / 2, line                     # eps / 2: the one rounding of z


# ---------------------------------------------------------------------------------------------------------------------
# 4. the box gate
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", [True, False])
def test_points_below_the_node_box_are_found_through_the_padded_box(bubble):
    geom = mesh_b(bubble)
    elem = np.array([0, 1])
    l = np.array([[0.25, 0.75], [0.75, 0.25]]) * (1 - 1e-3)
    pts = forward(geom, elem, l)
    assert pts[0, 1] < geom.x[:, 0, 1].min() == -0.1                           # below element 0's node box
    assert abs(pts[0, 0] - 0.74975) < 1e-4 and abs(pts[0, 1] + 0.11135) < 1e-4
    z = np.random.default_rng(4).standard_normal(geom.xflat.shape[0])
    vals, grads, found = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(found, elem), found
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))


# ---------------------------------------------------------------------------------------------------------------------
# 5. edges and outside
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", [True, False])
def test_shared_edges_take_the_lower_element_and_outside_is_nan(bubble):
    geom = mesh_a(bubble)
    t = geom.t                                                                 # (p, N) node ids; slot 1 is the node of edge l3 = 0
    owners = {}
    for e in range(t.shape[1]):
        for s in (1, 3, 5):
            owners.setdefault(int(t[s, e]), []).append(e)
    inner = [e for e in range(t.shape[1]) if len(owners[int(t[1, e])]) == 2]
    assert len(inner) >= 8
    rng = np.random.default_rng(55)
    elem = np.repeat(np.array(inner), 8)
    l1 = rng.uniform(0.1, 0.9, size=elem.size)                                 # off the corners, which more elements share
    pts = forward(geom, elem, np.stack([l1, 1.0 - l1], axis=1))                # l3 = 0
    lower = np.array([min(owners[int(t[1, e])]) for e in elem])
    assert (lower != elem).any() and (lower == elem).any()
    z = rng.standard_normal(geom.xflat.shape[0])
    vals, grads, found = m.interpolate(geom, z, pts, gradient=True, return_element=True)
    assert np.array_equal(found, lower), np.flatnonzero(found != lower)
    assert np.all(np.isfinite(vals)) and np.all(np.isfinite(grads))
    lo, hi = geom.xflat.min(axis=0), geom.xflat.max(axis=0)
    ext = hi - lo
    bad = np.array([[hi[0] + 0.5 * ext[0], 0.0], [0.0, lo[1] - 0.5 * ext[1]], [lo[0] - ext[0], hi[1] + ext[1]],
                    [np.nan, 0.1], [0.1, np.inf], [-np.inf, 0.0], [np.nan, np.nan]])
    v, g, e = m.interpolate(geom, z, bad, gradient=True, return_element=True)
    assert np.all(np.isnan(v)) and np.all(np.isnan(g)) and np.all(e == -1)
    v, e = m.interpolate(geom, z, bad, return_element=True)
    assert np.all(np.isnan(v)) and np.all(e == -1)


# ---------------------------------------------------------------------------------------------------------------------
# 6. PointLocator
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", [True, False])
def test_locator_is_bitwise_interpolate(bubble):
    geom = mesh_a(bubble)
    rng = np.random.default_rng(zlib.crc32(f"curvedloc{bubble}".encode()))
    pts = _mixed_points(geom, rng)
    n = geom.xflat.shape[0]
    with m.PointLocator(geom, pts) as loc:
        for _ in range(2):                                                     # two different z in a row
            z = rng.standard_normal(n)
            v1, g1, e1 = m.interpolate(geom, z, pts, gradient=True, return_element=True)
            assert _eq(loc.evaluate(z), v1)
            v, g = loc.evaluate(z, gradient=True)
            assert _eq(v, v1) and _eq(g, g1) and _eq(loc.elements, e1)
    assert np.isnan(v1).any() and (e1 < 0).any() and (e1 >= 0).sum() > e1.size // 2


# ---------------------------------------------------------------------------------------------------------------------
# 7. level curves and tessellation against the twins
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("refine", [None, 5], ids=["default", "r5"])
@pytest.mark.parametrize("bubble", [True, False])
def test_isocontour_and_tessellate_match_the_twins(bubble, refine):
    geom = mesh_a(bubble)
    p, N, d = geom.x.shape
    z, carry = smooth(geom.xflat)
    cr = carry[:, 0]                                                           # one carried field
    t = isocontour_twin(geom, z, LEVELS5, refine=refine, carry=cr)
    assert input_margin_ok(t, z), (refine, t.margin)
    c = m.isocontour(geom, z, LEVELS5, refine=refine, carry=cr)
    assert c.points.shape == (c.level.size, d, d) and c.points.dtype == np.float64
    assert c.level.size == t.level.size and c.level.size > 0
    assert np.array_equal(c.level, t.level) and np.array_equal(c.element, t.element)
    # the comparison of tests/test_gpu_contour.py ...
    amp = DEVICE_FACTOR * p * EPS * np.abs(z).max() / t.dv
    bound = amp * t.dx + 8 * EPS * np.abs(geom.xflat).max()
    ratio = float((np.abs(c.points - t.points).max(axis=2) / bound).max())
    cbound = amp[..., None] * t.dc + 8 * EPS * np.abs(cr).max()
    cratio = float((np.abs(c.carried - t.carried) / cbound).max())
    bits = bool(np.array_equal(c.points, t.points) and np.array_equal(c.carried, t.carried))
    line = (f"curved fem2d_P2 isocontour vs twin bubble={bubble} refine={refine}: S = {c.level.size}, points error / bound "
            f"{ratio:.3e}, carried error / bound {cratio:.3e}, bitwise {bits}")
    print(line)
    record_observation(line)
    assert ratio <= 1.0 and cratio <= 1.0, line
    assert np.allclose(c.measure(), t.measure(), rtol=1e-9, atol=0)
    # ... and to the bit: neither side contracts a multiplication with an addition
    assert bits, line
    r = 2 if refine is None else refine
    F = np.stack([z, cr], axis=1)
    tt = tessellate_twin(geom, F, refine)
    ct = m.tessellate(geom, F, refine=refine)
    assert ct.points.shape == (N * r * r, 3, 2) and tt.points.shape == ct.points.shape and ct.points.shape[0] > 0
    assert np.array_equal(ct.element, tt.element)
    tratio = float(np.abs(ct.points - tt.points).max() / (DEVICE_FACTOR * p * EPS * np.abs(geom.xflat).max()))
    vratio = float((np.abs(ct.values - tt.values).max(axis=(0, 1)) / (DEVICE_FACTOR * p * EPS * np.abs(F).max(axis=0))).max())
    tbits = bool(np.array_equal(ct.points, tt.points) and np.array_equal(ct.values, tt.values))
    line = (f"curved fem2d_P2 tessellate vs twin bubble={bubble} refine={refine}: T = {ct.points.shape[0]}, points error / "
            f"bound {tratio:.3e}, values error / bound {vratio:.3e}, bitwise {tbits}")
    print(line)
    record_observation(line)
    assert tratio <= 1.0 and vratio <= 1.0, line
    assert np.isclose(ct.measure(), tt.measure(), rtol=1e-9, atol=0)
    assert tbits, line


# ---------------------------------------------------------------------------------------------------------------------
# 8. field lines against the twin
# ---------------------------------------------------------------------------------------------------------------------

def _line_field(X, mode):
    """The fields of tests/test_streamlines.py with coefficients under which most lines stay: `vector_field` and
    `scalar_field` themselves leave fewer than half of the 257 twin lines with 10 points on this mesh (observed: 105 and
    101; 80 of the seeds lie outside).  Vector: the rotation about the origin with an inward part (lines spiral in and
    stall near the origin); gradient: a drift along (0.4, 0.15) whose speed stays above GPU_MIN_SPEED (lines cross the
    mesh and leave on the far side).  Both keep a non-polynomial term."""
    x, y = X[:, 0], X[:, 1]
    if mode == "vector":
        return np.stack([-y - 0.7 * x + 0.1 * np.sin(2.0 * x), x - 0.7 * y + 0.1 * np.sin(2.0 * y)], axis=1)
    return 0.4 * x + 0.15 * y + 0.05 * np.sin(1.5 * x + 0.5 * y)


@pytest.mark.parametrize("mode", ["gradient", "vector"])
@pytest.mark.parametrize("bubble", [True, False])
def test_streamlines_are_bitwise_the_twins(bubble, mode):
    geom = mesh_a(bubble)
    z = _line_field(geom.xflat, mode)
    seeds = gpu_seeds(2, 257)
    twin = trace_twin(interpolated(geom, z, mode), seeds, GPU_STEP[False], GPU_MAX_STEPS, normalize=False,
                      min_speed=GPU_MIN_SPEED)
    long_lines = int(np.count_nonzero(twin.n >= 10))
    print(f"curved fem2d_P2 streamlines bubble={bubble} {mode}: {long_lines} of {seeds.shape[0]} twin lines have >= 10 points; "
          f"MAX_STEPS/LEFT/STALLED/OUTSIDE = {list(np.bincount(twin.status, minlength=4))}")
    assert 2 * long_lines >= seeds.shape[0]                                    # a condition on the twin alone
    with StreamTracer(geom, z, field=mode) as st:
        got = st.trace(seeds, step=GPU_STEP[False], max_steps=GPU_MAX_STEPS, normalize=False, min_speed=GPU_MIN_SPEED)
    assert np.array_equal(got.n, twin.n), np.flatnonzero(got.n != twin.n)
    assert np.array_equal(got.status, twin.status), np.flatnonzero(got.status != twin.status)
    assert same(got, twin)


# ---------------------------------------------------------------------------------------------------------------------
# 9. end to end: refine, solve, evaluate
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", [True, False])
def test_solve_on_a_refined_curved_mesh_and_evaluate(bubble):
    from oracle import mgb_oracle
    g2 = m.subdivide(mesh_a(bubble), 2)
    assert g2.x.shape[1] == 128 and g2.discretization.curved
    prob = m.assemble(m.amg(g2), p=1.5)
    sol = m.mgb_solve(prob)
    assert_z_close(sol.z, mgb_oracle.mgb_solve(prob)["z"], f"curved fem2d_P2 L=2 bubble={bubble} p=1.5")
    elem, made, pts = manufactured(g2, np.random.default_rng(9), 1000)
    vals, found = m.interpolate(g2, sol.z[:, 0], pts, return_element=True)
    assert np.array_equal(found, elem) and np.all(np.isfinite(vals))
