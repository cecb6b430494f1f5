"""RayCaster / render_volume on the device against the NumPy twin (tests/raycast_twin.py).

The twin places the samples by the same IEEE operations as the kernels, so `offsets`, `step_of_ray` and `samples()` must
agree bit for bit once no ray has (tmax - tmin)/step so close to a half-integer that two roundings could give different
counts (asserted first, on the twin alone; the cases live in tests/test_raycast.py, where that check also runs without a
GPU).  The twin takes its sample values from `interpolate()` at its own samples, which is pinned elsewhere and gives NaN
outside the mesh; the caster evaluates at the element and reference point it stored, as `PointLocator` does.

- `integrate`: both sides add bitwise-equal values in the same order (n_r additions, one multiplication), so the
  expected difference is 0; the bound is 16 (n_r + 1) eps max|z| (tmax - tmin) per ray.
- `render`: the two sides differ only in their `exp`, at most 1 ulp each per step, which propagates linearly through
  T; the bound is 16 (n_r + 1) eps max(1, max|transfer colour|) per channel.
"""
import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd.raycast import RayCaster, camera_rays, render_volume
from raycast_twin import clip_box_twin, default_transfer_twin, integrate_twin, rays_twin, render_twin
from test_raycast import (CLIM, CUBE, EPS, EYE, GPU_CASES, HALF_INTEGER_MARGIN, TABLE5, axis_rays, case_twin, centre_rays,
                          closed_form, linear, render_bound, smooth)

pytestmark = pytest.mark.gpu


@pytest.fixture(params=sorted(GPU_CASES), scope="module")
def case(request):
    """One caster per case, shared by the tests of the case, with the twin and the values interpolate() gives at the
    twin's samples (computed once, never modified)."""
    name = request.param
    geom, o, d, step, t_min, t_max, t = case_twin(name)
    assert t.half_integer_margin() > HALF_INTEGER_MARGIN, (name, t.half_integer_margin())
    Z = smooth(geom.xflat)
    vals, elem = m.interpolate(geom, Z, t.pts, return_element=True)
    vals.setflags(write=False)
    with RayCaster(geom, o, d, step, t_min=t_min, t_max=t_max) as rc:
        yield name, geom, (o, d, step, t_min, t_max), t, Z, vals, elem, rc


def test_samples_are_bitwise_the_twins(case):
    name, geom, _, t, _, _, _, rc = case
    assert rc.nrays == t.n.size and rc.nsamples == t.pts.shape[0] > 0
    off = rc.offsets
    assert off.dtype == np.int64 and np.array_equal(off, t.offsets), name
    assert np.array_equal(rc.step_of_ray, t.h), name
    pts = rc.samples()
    assert pts.shape == t.pts.shape and pts.dtype == np.float64 and np.array_equal(pts, t.pts), name


def test_length_counts_the_samples_in_elements(case):
    name, _, _, t, _, _, elem, rc = case
    inside = np.concatenate([[0], np.cumsum(elem >= 0)])
    count = inside[t.offsets[1:]] - inside[t.offsets[:-1]]
    if name in ("fem3d_k2", "fem3d_k3", "fem3d_k2_curved", "fem2d_k2"):
        assert (elem < 0).any() and (count < t.n).any(), "a widened box has samples outside the mesh"
    assert np.array_equal(rc.length, t.h * count), name


def test_integrate_matches_the_twin(case):
    name, _, _, t, Z, vals, _, rc = case
    got = rc.integrate(Z)
    want = integrate_twin(t, vals)
    assert got.shape == want.shape == (t.n.size, 3)
    bound = 16 * (t.n + 1) * EPS * np.abs(Z).max() * t.chord
    ratio = np.abs(got - want)[t.n > 0] / bound[t.n > 0, None]
    record_observation(f"raycast integrate {name}: max difference / bound {ratio.max():.3e}")
    print(f"{name}: integrate max difference / bound {ratio.max():.3e}")
    assert (np.abs(got - want) <= bound[:, None]).all(), (name, ratio.max())
    assert np.array_equal(got[t.n == 0], np.zeros(((t.n == 0).sum(), 3)))
    for c in range(3):                                        # column by column bitwise the single-column call
        one = rc.integrate(Z[:, c])
        assert one.shape == (t.n.size,) and np.array_equal(one, got[:, c]), (name, c)


@pytest.mark.parametrize("which", ["table5", "default"])
def test_render_matches_the_twin(case, which):
    name, geom, _, t, Z, vals, _, rc = case
    u = Z[:, 0]
    if which == "table5":
        table, clim = TABLE5, CLIM
        got = rc.render(u, TABLE5, CLIM)
    else:
        table, clim = default_transfer_twin(clip_box_twin(geom)), (float(u.min()), float(u.max()))
        got = rc.render(u)
    want = render_twin(t, vals[:, 0], table, *clim)
    assert got.shape == (t.n.size, 4) and got.dtype == np.float64
    bound = render_bound(t.n, table)
    ratio = np.abs(got - want) / bound[:, None]
    record_observation(f"raycast render {name} {which}: max difference / bound {ratio.max():.3e}")
    print(f"{name} {which}: render max difference / bound {ratio.max():.3e}")
    assert (np.abs(got - want) <= bound[:, None]).all(), (name, which, ratio.max())
    assert np.array_equal(got[t.n == 0], np.zeros(((t.n == 0).sum(), 4)))
    assert (got[t.n > 0, 3] > 0).any() and (got[:, 3] <= 1.0).all()


def test_reuse_and_determinism(case):
    name, geom, (o, d, step, t_min, t_max), t, Z, _, _, rc = case
    u = Z[:, 0]
    a = rc.render(u, TABLE5, CLIM)
    assert np.array_equal(a, rc.render(u, TABLE5, CLIM)), name
    rc.integrate(Z[:, :2])                                    # another ncomp in between
    b = rc.render(u, TABLE5, CLIM)
    with RayCaster(geom, o, d, step, t_min=t_min, t_max=t_max) as fresh:
        c = fresh.render(u, TABLE5, CLIM)
        assert np.array_equal(fresh.offsets, rc.offsets)
    assert np.array_equal(a, b) and np.array_equal(b, c), name
    # NaN in u: the samples it reaches contribute nothing, the result stays finite
    un = u.copy()
    un[: geom.x.shape[0]] = np.nan                            # the nodes of element 0
    r = rc.render(un, TABLE5, CLIM)
    assert np.isfinite(r).all()


# ---------------------------------------------------------------------------------------------------------------------
# exactness on the device: the k = 1 cube
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def cube():
    return m.subdivide(m.fem3d(k=1), 1)


def test_linear_field_integrals_and_chords_are_exact(cube):
    assert np.array_equal(clip_box_twin(cube), CUBE)
    o, d, mid = axis_rays()
    u = linear(cube.xflat)
    with RayCaster(cube, o, d, 2.0 / 8.0) as rc:
        assert np.array_equal(rc.offsets, 8 * np.arange(13)) and np.array_equal(rc.step_of_ray, np.full(12, 0.25))
        I = rc.integrate(u)
        L = rc.length
    scale = np.abs(u).max()
    print(f"linear field: max error / (64 eps max|u|) {np.abs(I - 2.0 * linear(mid)).max() / (64 * EPS * scale):.3e}")
    assert np.abs(I - 2.0 * linear(mid)).max() <= 64 * EPS * scale
    assert np.abs(L - 2.0).max() <= 64 * EPS
    o, d, chord = centre_rays()
    with RayCaster(cube, o, d, 0.13) as rc:
        assert np.abs(rc.length - chord).max() <= 64 * EPS * chord.max()


def test_constant_field_render_is_the_closed_form(cube):
    o, d, chord = centre_rays()
    t = rays_twin(CUBE, o, d, 0.13)
    n = cube.xflat.shape[0]
    with RayCaster(cube, o, d, 0.13) as rc:
        assert np.array_equal(rc.offsets, t.offsets)
        for c in (0.31, -0.9, 2.0):
            got = rc.render(np.full(n, c), TABLE5, CLIM)
            want = closed_form(TABLE5, CLIM, c, chord)
            ratio = np.abs(got - want) / render_bound(t.n, TABLE5)[:, None]
            print(f"constant field {c}: max difference / bound {ratio.max():.3e}")
            assert (ratio <= 1.0).all(), (c, ratio.max())


# ---------------------------------------------------------------------------------------------------------------------
# render_volume, misses, the sample limit
# ---------------------------------------------------------------------------------------------------------------------

def test_render_volume_is_the_caster_on_camera_rays():
    geom = m.subdivide(m.fem3d(k=2), 1)
    u = smooth(geom.xflat)[:, 0]
    W, H = 7, 5
    step = 0.21
    img = render_volume(geom, u, EYE, (0.1, 0.0, -0.1), size=(W, H), fov=35.0, step=step, transfer=TABLE5, clim=CLIM)
    o, d = camera_rays(EYE, (0.1, 0.0, -0.1), size=(W, H), fov=35.0)
    with RayCaster(geom, o, d, step) as rc:
        assert rc.nsamples > 0 and np.diff(rc.offsets).max() <= 64
        ref = rc.render(u, TABLE5, CLIM)
    assert img.shape == (H, W, 4) and img.dtype == np.float64
    assert np.array_equal(img, ref.reshape(H, W, 4))
    assert img[H // 2, W // 2, 3] > 0.0, "the centre pixel sees the mesh"


def test_rays_that_all_miss():
    geom = m.subdivide(m.fem3d(k=2), 1)
    o = np.array([[5.0, 5.0, 5.0], [-3.0, 2.5, 0.0], [0.0, 0.0, 4.0]])
    d = np.array([[1.0, 0.2, 0.1], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    Z = smooth(geom.xflat)
    with RayCaster(geom, o, d, 0.1) as rc:
        assert rc.nsamples == 0 and np.array_equal(rc.offsets, np.zeros(4, dtype=np.int64))
        assert np.array_equal(rc.step_of_ray, np.zeros(3)) and np.array_equal(rc.length, np.zeros(3))
        assert rc.samples().shape == (0, 3)
        assert np.array_equal(rc.integrate(Z), np.zeros((3, 3)))
        assert np.array_equal(rc.render(Z[:, 0]), np.zeros((3, 4)))


def test_too_many_samples_are_refused_by_count():
    geom = m.fem3d(k=1)
    o, d, _ = axis_rays()
    with pytest.raises(ValueError, match=r"S = \d+ samples exceed 2\^31 - 1"):
        RayCaster(geom, o, d, 1e-8)                           # 12 rays of 2e8 samples: refused after the count pass
