"""RayCaster / camera_rays / render_volume on the CPU: the camera's geometry and its documented pixel order, every
argument check raised before the library is touched, empty input without a device, and the NumPy twin
(tests/raycast_twin.py) the GPU tests compare against, itself checked against exact answers with an exact field standing
in for `interpolate()`.  The cases of tests/test_gpu_raycast.py are defined here, so that their input condition (no ray
whose (tmax - tmin)/step lies within 1e-6 of a half-integer, where two roundings could legitimately give different
sample counts) is checked without a GPU, on the twin alone.
"""
import math

import numpy as np
import pytest

import mgb_amd as m
from mgb_amd.raycast import RayCaster, camera_rays, clip_box, default_transfer, render_volume
from raycast_twin import (clip_box_twin, default_transfer_twin, diagonal_twin, integrate_twin, rays_twin, render_twin)

EPS = float(np.finfo(np.float64).eps)
HALF_INTEGER_MARGIN = 1e-6

# a fixed non-monotone table: r, g, b, sigma per row
TABLE5 = np.array([[0.9, 0.1, 0.0, 0.00],
                   [0.2, 0.8, 0.3, 1.70],
                   [0.0, 0.4, 1.0, 0.25],
                   [1.0, 1.0, 0.2, 2.40],
                   [0.3, 0.0, 0.7, 0.60]])
CLIM = (-0.55, 0.85)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_raycast.py
# ---------------------------------------------------------------------------------------------------------------------

def _curve3(X):
    """A smooth, non-polynomial map of [-1, 1]^3 applied to every node."""
    Y = X.copy()
    Y[..., 0] += 0.08 * np.sin(np.pi * X[..., 1])
    Y[..., 1] += 0.06 * np.sin(np.pi * X[..., 0]) * X[..., 2]
    Y[..., 2] += 0.05 * np.cos(np.pi * X[..., 0]) * X[..., 1]
    return Y


EYE = (2.7, -3.1, 1.9)


def rays3d():
    """Perspective rays (some miss at the corners of the image), axis-parallel rays (hits and a miss), rays with one zero
    component, rays that point away, rays that start inside."""
    o, d = camera_rays(EYE, (0.0, 0.0, 0.0), size=(6, 5), fov=40.0)
    extra = [
        ((-3.0, 0.3, -0.2), (1.0, 0.0, 0.0)),
        ((0.4, 5.0, 0.1), (0.0, -2.0, 0.0)),
        ((0.1, 0.2, -4.0), (0.0, 0.0, 1.0)),
        ((-3.0, 2.5, 0.0), (1.0, 0.0, 0.0)),        # parallel to x, outside in y: misses
        ((-2.5, -2.2, 0.35), (1.0, 0.9, 0.0)),      # one zero component
        ((0.2, -3.0, -2.0), (0.0, 1.0, 0.7)),
        ((5.0, 5.0, 5.0), (1.0, 0.2, 0.1)),         # points away: misses
        ((-4.0, 0.0, 3.5), (1.0, 0.1, 0.0)),        # passes above the box: misses
        ((0.1, -0.2, 0.3), (0.3, 0.5, -0.4)),       # starts inside
        ((0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),         # starts inside, on element faces
        ((-0.6, 0.7, -0.5), (-0.2, -1.0, 0.6)),     # starts inside
    ]
    return (np.concatenate([o, np.array([e[0] for e in extra])]),
            np.concatenate([d, np.array([e[1] for e in extra])]))


def rays2d():
    """A fan from one point (some of it misses), axis-parallel rays, misses, rays that start inside."""
    apex = np.array([2.3, -1.7])
    fan = np.stack([np.array([-1.0 + 0.37 * i, 1.9 - 0.41 * i]) - apex for i in range(9)])
    extra = [
        ((-3.0, 0.3), (1.0, 0.0)),
        ((0.4, 2.5), (0.0, -3.0)),
        ((-3.0, 1.6), (1.0, 0.0)),                  # parallel to x, outside in y: misses
        ((3.0, 3.0), (1.0, 0.3)),                   # points away: misses
        ((0.1, -0.2), (0.3, 0.5)),                  # starts inside
        ((0.0, 0.0), (1.0, 0.0)),                   # starts inside, along an element edge
        ((-0.6, 0.7), (-0.2, -1.0)),                # starts inside
    ]
    return (np.concatenate([np.tile(apex, (9, 1)), np.array([e[0] for e in extra])]),
            np.concatenate([fan, np.array([e[1] for e in extra])]))


# name -> (geometry, rays, step, t_min, t_max): t_max cuts the rays that come from far away short
GPU_CASES = {
    "fem3d_k1": (lambda: m.subdivide(m.fem3d(k=1), 1), rays3d, 0.13, 0.02, 4.6),
    "fem3d_k2": (lambda: m.subdivide(m.fem3d(k=2), 1), rays3d, 0.13, 0.02, 4.6),
    "fem3d_k3": (lambda: m.subdivide(m.fem3d(k=3), 1), rays3d, 0.13, 0.02, 4.6),
    "fem3d_k2_curved": (lambda: m.fem3d(k=2, K=_curve3(m.fem3d(k=2).x)), rays3d, 0.13, 0.02, 4.6),
    "fem2d_k2": (lambda: m.subdivide(m.fem2d(k=2), 1), rays2d, 0.11, 0.02, 3.4),
    "fem2d_P2": (lambda: m.subdivide(m.fem2d_P2(), 1), rays2d, 0.11, 0.02, 3.4),
    "fem2d_P1": (lambda: m.subdivide(m.fem2d_P1(), 1), rays2d, 0.11, 0.02, 3.4),
}


def smooth(X):
    """(p*N, 3): smooth non-polynomial functions of the node coordinates; column 0 is the one that is rendered."""
    x, y = X[:, 0], X[:, 1]
    w = X[:, 2] if X.shape[1] == 3 else np.zeros_like(x)
    return np.stack([np.sin(1.3 * x + 0.4) * np.cos(0.9 * y - 0.2) + 0.35 * np.sin(1.1 * w + 0.3),
                     np.exp(0.5 * x - 0.3 * y + 0.2 * w),
                     np.cos(x + 2.0 * y - w)], axis=1)


def case_twin(name):
    make, rays, step, t_min, t_max = GPU_CASES[name]
    geom = make()
    o, d = rays()
    return geom, o, d, step, t_min, t_max, rays_twin(clip_box_twin(geom), o, d, step, t_min, t_max)


@pytest.mark.parametrize("name", sorted(GPU_CASES))
def test_gpu_cases_meet_the_input_condition_on_the_twin(name):
    geom, o, d, step, t_min, t_max, t = case_twin(name)
    print(f"{name}: R = {t.n.size}, S = {t.pts.shape[0]}, max n = {t.n.max()}, margin {t.half_integer_margin():.3e}")
    assert t.half_integer_margin() > HALF_INTEGER_MARGIN
    assert t.n.size <= 64 and t.n.max() <= 64
    # the mix every case is meant to have
    assert (t.n == 0).any() and (t.n > 0).any(), "hits and misses"
    assert ((t.dn == 0.0).any(axis=1) & (t.n > 0)).any(), "an axis-parallel ray that hits"
    assert ((t.dn == 0.0).any(axis=1) & (t.n == 0)).any(), "an axis-parallel ray that misses"
    assert ((t.tmin == t_min) & (t.n > 0)).any(), "a ray that starts inside the box"
    assert ((t.tmin + t.chord == t_max) & (t.n > 0)).any(), "a ray t_max cuts short"
    assert ((t.tmin + t.chord < t_max) & (t.n > 0)).any(), "a ray t_max does not cut"


def test_the_twin_restates_the_modules_host_side():
    for name in sorted(GPU_CASES):
        geom = GPU_CASES[name][0]()
        assert np.array_equal(clip_box(geom), clip_box_twin(geom)), name
        assert np.array_equal(default_transfer(diagonal_twin(clip_box_twin(geom))),
                              default_transfer_twin(clip_box_twin(geom))), name
    assert np.array_equal(clip_box(m.fem3d(k=1))[1] - clip_box(m.fem3d(k=1))[0], [2.0, 2.0, 2.0])
    assert np.array_equal(clip_box(m.fem3d(k=2))[1] - clip_box(m.fem3d(k=2))[0], [2.5, 2.5, 2.5])
    assert np.array_equal(clip_box(m.fem2d_P2())[1] - clip_box(m.fem2d_P2())[0], [2.0, 2.0])


# ---------------------------------------------------------------------------------------------------------------------
# camera_rays
# ---------------------------------------------------------------------------------------------------------------------

def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_names_are_exported():
    assert m.RayCaster is RayCaster and m.camera_rays is camera_rays and m.render_volume is render_volume


def test_centre_ray_points_at_the_target():
    eye, target = np.array(EYE), np.array([0.2, -0.1, 0.3])
    o, d = camera_rays(eye, target, size=(5, 3), fov=35.0)
    assert o.shape == d.shape == (15, 3)
    assert np.array_equal(o, np.tile(eye, (15, 1)))
    c = d[1 * 5 + 2]                                           # row 1 of 3, column 2 of 5: the centre pixel
    assert np.abs(_unit(c) - _unit(target - eye)).max() <= 8 * EPS
    # RayCaster normalises: the directions it uses have unit length
    dn = rays_twin(np.array([[-1.0] * 3, [1.0] * 3]), o, d, 0.1).dn
    assert np.abs(np.linalg.norm(dn, axis=1) - 1.0).max() <= 4 * EPS


@pytest.mark.parametrize("fov", [20.0, 30.0, 75.0])
def test_corner_rays_subtend_fov_vertically(fov):
    # with H rows the centres of the top and the bottom row are (H - 1)/H of the image height apart
    W, H = 4, 6
    _, d = camera_rays(EYE, (0, 0, 0), size=(W, H), fov=fov)
    d = d.reshape(H, W, 3)
    fwd = _unit(-np.array(EYE))
    top = 0.5 * (d[0, 0] + d[0, W - 1])                        # the middle of the top row's centres
    bot = 0.5 * (d[H - 1, 0] + d[H - 1, W - 1])
    half = math.tan(math.radians(fov) / 2.0) * (H - 1) / H
    for v in (top, bot):
        tangent = np.linalg.norm(v - np.dot(v, fwd) * fwd) / np.dot(v, fwd)
        assert abs(tangent - half) <= 16 * EPS * max(1.0, half)
    # and the two edges of the image itself subtend fov: extrapolate half a pixel
    edge = top + 0.5 * (top - bot) / (H - 1)
    ang = math.degrees(math.atan(np.linalg.norm(edge - np.dot(edge, fwd) * fwd) / np.dot(edge, fwd)))
    assert abs(2 * ang - fov) <= 1e-12 * fov


def test_row_and_column_order():
    # looking along +y with z up: x grows to the right.  Ray r = row * W + col; row 0 is the top, column 0 the left.
    W, H = 4, 3
    _, d = camera_rays((0, -5, 0), (0, 0, 0), up=(0, 0, 1), size=(W, H), fov=30.0)
    d = d.reshape(H, W, 3)
    assert (np.diff(d[:, :, 0], axis=1) > 0).all(), "x grows with the column"
    assert (np.diff(d[:, :, 2], axis=0) < 0).all(), "z falls with the row"
    assert np.abs(d[:, :, 1] - 1.0).max() <= 4 * EPS
    assert np.allclose(d[:, ::-1, 0], -d[:, :, 0], rtol=0, atol=4 * EPS)
    assert np.allclose(d[::-1, :, 2], -d[:, :, 2], rtol=0, atol=4 * EPS)
    # pixels are square: the horizontal pitch equals the vertical one
    assert abs((d[0, 1, 0] - d[0, 0, 0]) - (d[0, 0, 2] - d[1, 0, 2])) <= 8 * EPS


def test_orthographic_rays():
    W, H, height = 3, 5, 2.4
    o, d = camera_rays(EYE, (0, 0, 0), size=(W, H), height=height)
    fwd = _unit(-np.array(EYE))
    assert np.abs(d - fwd).max() <= 4 * EPS and np.array_equal(d, np.tile(d[0], (W * H, 1)))
    o = o.reshape(H, W, 3)
    # the top and the bottom row's centres are height (H - 1)/H apart, perpendicular to the view
    span = o[0, 1] - o[H - 1, 1]
    assert abs(np.linalg.norm(span) - height * (H - 1) / H) <= 16 * EPS * height
    assert abs(np.dot(span, fwd)) <= 16 * EPS * height
    assert span[2] > 0, "row 0 is the top (up = +z)"
    assert np.abs(o[2, 1] - np.array(EYE)).max() <= 8 * EPS * 4, "the centre pixel starts at the eye"


@pytest.mark.parametrize("size", [(0, 3), (3, 0), (2.5, 3), (True, 3), (3,), "ab", None, (-1, 2)])
def test_bad_sizes_are_refused(size):
    with pytest.raises(ValueError, match="camera_rays: size"):
        camera_rays(EYE, (0, 0, 0), size=size)


def test_bad_cameras_are_refused():
    with pytest.raises(ValueError, match="eye and target coincide"):
        camera_rays(EYE, EYE)
    with pytest.raises(ValueError, match="up is parallel"):
        camera_rays((0, 0, 3), (0, 0, 0), up=(0, 0, 1))
    with pytest.raises(ValueError, match="fov must be"):
        camera_rays(EYE, (0, 0, 0), fov=180.0)
    with pytest.raises(ValueError, match="height must be"):
        camera_rays(EYE, (0, 0, 0), height=0.0)
    with pytest.raises(ValueError, match="eye must be three finite"):
        camera_rays((0, np.nan, 1), (0, 0, 0))
    with pytest.raises(ValueError, match="target must be three finite"):
        camera_rays(EYE, (0, 0))


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


O3, D3 = np.array([[-3.0, 0.1, 0.2]]), np.array([[1.0, 0.0, 0.0]])


@pytest.mark.parametrize("geom,name", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
])
def test_unsupported_families_are_refused_by_name(no_library, geom, name):
    d = geom.xflat.shape[1]
    with pytest.raises(ValueError, match=rf"RayCaster: {name} geometries are not supported"):
        RayCaster(geom, np.zeros((1, d)), np.ones((1, d)), 0.1)


def test_embedded_manifold_is_refused(no_library):
    geom = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)     # a segment in the plane
    with pytest.raises(ValueError, match=r"RayCaster: fem1d embedded in 2 dimensions"):
        RayCaster(geom, np.zeros((1, 2)), np.ones((1, 2)), 0.1)


def test_curved_p2_is_refused(no_library):
    K = m.fem2d_P2().x.copy()
    K[1, 0, :] += 0.05                                                     # an edge node off its edge's midpoint
    with pytest.raises(ValueError, match=r"fem2d_P2 .* straight elements"):
        RayCaster(m.fem2d_P2(K=K), np.zeros((1, 2)), np.ones((1, 2)), 0.1)


def test_render_volume_is_3d_only(no_library):
    geom = m.fem2d(k=1)
    with pytest.raises(ValueError, match=r"render_volume: fem2d geometries are not supported"):
        render_volume(geom, np.zeros(_n(geom)), EYE, (0, 0, 0))
    with pytest.raises(ValueError, match=r"render_volume: spectral2d geometries are not supported"):
        render_volume(m.spectral2d(n=4), np.zeros(16), EYE, (0, 0, 0))


@pytest.mark.parametrize("o,d,match", [
    (np.zeros((2, 3)), np.ones((3, 3)), "o and d must both be"),
    (np.zeros((2, 2)), np.ones((2, 2)), "o and d must both be"),
    (np.zeros((2, 3, 1)), np.ones((2, 3, 1)), "o and d must both be"),
    (np.zeros(3), np.ones((1, 3)), "o and d must both be"),
    (np.array([[0.0, np.nan, 0.0]]), D3, "origin must be finite"),
    (np.array([[0.0, np.inf, 0.0]]), D3, "origin must be finite"),
    (O3, np.array([[1.0, np.nan, 0.0]]), "direction must be finite"),
    (O3, np.array([[-np.inf, 0.0, 0.0]]), "direction must be finite"),
    (O3, np.zeros((1, 3)), "direction is zero"),
    (np.tile(O3, (2, 1)), np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]), "direction is zero"),
    (O3, np.array([[1e-200, 0.0, 0.0]]), "too long or too short"),
    (O3, np.array([[1e200, 1e200, 0.0]]), "too long or too short"),
])
def test_bad_rays_are_refused(no_library, o, d, match):
    with pytest.raises(ValueError, match=match):
        RayCaster(m.fem3d(k=1), o, d, 0.1)


@pytest.mark.parametrize("kw,match", [
    (dict(step=0.0), "step must be finite and positive"),
    (dict(step=-0.1), "step must be finite and positive"),
    (dict(step=np.nan), "step must be finite and positive"),
    (dict(step=np.inf), "step must be finite and positive"),
    (dict(step="x"), "must be numbers"),
    (dict(step=0.1, t_min=np.inf), "t_min must be finite"),
    (dict(step=0.1, t_min=np.nan), "t_min must be finite"),
    (dict(step=0.1, t_min=1.0, t_max=1.0), "t_max must be greater than t_min"),
    (dict(step=0.1, t_min=1.0, t_max=0.5), "t_max must be greater than t_min"),
    (dict(step=0.1, t_max=np.nan), "t_max must be greater than t_min"),
])
def test_bad_steps_and_ranges_are_refused(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        RayCaster(m.fem3d(k=1), O3, D3, **kw)


@pytest.fixture
def empty_caster(no_library):
    geom = m.subdivide(m.fem3d(k=2), 1)
    with RayCaster(geom, np.zeros((0, 3)), np.zeros((0, 3)), 0.1) as rc:
        yield geom, rc


def test_no_rays_need_no_device(empty_caster):
    geom, rc = empty_caster
    n = _n(geom)
    assert rc.nrays == 0 and rc.nsamples == 0
    assert rc.offsets.dtype == np.int64 and np.array_equal(rc.offsets, [0])
    assert rc.step_of_ray.shape == (0,) and rc.length.shape == (0,)
    assert rc.samples().shape == (0, 3)
    assert rc.integrate(np.zeros(n)).shape == (0,) and rc.integrate(np.zeros((n, 3))).shape == (0, 3)
    r = rc.render(geom.xflat[:, 0])
    assert r.shape == (0, 4) and r.dtype == np.float64


def test_bad_fields_are_refused(empty_caster):
    geom, rc = empty_caster
    n = _n(geom)
    u = geom.xflat[:, 0]
    with pytest.raises(ValueError, match=rf"needs {n} values"):
        rc.integrate(np.zeros(n + 1))
    with pytest.raises(ValueError, match="vector or a matrix"):
        rc.integrate(np.zeros((n, 1, 1)))
    with pytest.raises(ValueError, match=rf"u must be a vector of {n} values"):
        rc.render(np.zeros((n, 2)))
    with pytest.raises(ValueError, match=rf"u must be a vector of {n} values"):
        rc.render(np.zeros(n - 1))
    for bad in (np.zeros((1, 4)), np.zeros((5, 3)), np.zeros(8), np.zeros((2, 4, 1))):
        with pytest.raises(ValueError, match=r"transfer must be \(K, 4\) with K >= 2"):
            rc.render(u, bad)
    T = TABLE5.copy()
    T[2, 1] = np.nan
    with pytest.raises(ValueError, match="transfer entry must be finite"):
        rc.render(u, T)
    T = TABLE5.copy()
    T[3, 3] = -1e-3
    with pytest.raises(ValueError, match="sigma must be >= 0"):
        rc.render(u, T)
    for clim in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.inf), (1.0,), 3.0, "ab"):
        with pytest.raises(ValueError, match="clim must be"):
            rc.render(u, TABLE5, clim)
    with pytest.raises(ValueError, match="u is constant"):
        rc.render(np.full(n, 0.25))
    with pytest.raises(ValueError, match="no finite entry"):
        rc.render(np.full(n, np.nan))
    rc.close()
    with pytest.raises(ValueError, match="closed"):
        rc.render(u)


def test_render_volume_checks_before_device_work(no_library):
    geom = m.fem3d(k=1)
    n = _n(geom)
    u = geom.xflat[:, 0]
    with pytest.raises(ValueError, match=rf"u must be a vector of {n} values"):
        render_volume(geom, np.zeros(n + 2), EYE, (0, 0, 0), size=(2, 2))
    with pytest.raises(ValueError, match="clim must be"):
        render_volume(geom, u, EYE, (0, 0, 0), size=(2, 2), clim=(1.0, 0.0))
    with pytest.raises(ValueError, match="u is constant"):
        render_volume(geom, np.ones(n), EYE, (0, 0, 0), size=(2, 2))
    with pytest.raises(ValueError, match=r"transfer must be \(K, 4\)"):
        render_volume(geom, u, EYE, (0, 0, 0), size=(2, 2), transfer=np.zeros((1, 4)))
    with pytest.raises(ValueError, match="camera_rays: size"):
        render_volume(geom, u, EYE, (0, 0, 0), size=(2, 0))
    with pytest.raises(ValueError, match="step must be finite and positive"):
        render_volume(geom, u, EYE, (0, 0, 0), size=(2, 2), step=0.0)


# ---------------------------------------------------------------------------------------------------------------------
# the twin against exact answers (an exact field stands in for interpolate())
# ---------------------------------------------------------------------------------------------------------------------

CUBE = np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
LIN = np.array([0.7, -0.4, 0.3])
LIN0 = 0.15


def linear(X):
    return LIN0 + X @ LIN


def axis_rays():
    """Axis-parallel rays through [-1, 1]^3 from outside, two per axis and direction: (o, d, the chord's midpoint)."""
    o, d, mid = [], [], []
    for a in range(3):
        for sign in (1.0, -1.0):
            for b, c in ((0.3, -0.45), (-0.8, 0.65)):
                p = np.zeros(3)
                p[(a + 1) % 3], p[(a + 2) % 3] = b, c
                e = np.zeros(3)
                e[a] = sign
                o.append(p - 3.0 * e)
                d.append(2.5 * e)                  # not normalised
                mid.append(p)
    return np.array(o), np.array(d), np.array(mid)


def centre_rays():
    """Oblique rays through the centre of [-1, 1]^3 from outside: the chord is 2 / max|d| for the unit direction d."""
    dirs = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0], [2.0, 1.0, 0.0], [0.3, -1.0, 0.5], [-0.7, 0.2, 1.0], [1.0, 0.0, 0.0]])
    dn = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    return -3.0 * dn, dirs, 2.0 / np.abs(dn).max(axis=1)


def test_twin_integrates_a_linear_field_exactly():
    o, d, mid = axis_rays()
    t = rays_twin(CUBE, o, d, 2.0 / 8.0)
    assert np.array_equal(t.n, np.full(12, 8)) and np.array_equal(t.h, np.full(12, 0.25))
    vals = linear(t.pts)
    scale = np.abs(vals).max()
    I = integrate_twin(t, vals)
    assert np.abs(I - 2.0 * linear(mid)).max() <= 64 * EPS * scale
    L = integrate_twin(t, np.ones(t.pts.shape[0]))
    assert np.abs(L - 2.0).max() <= 64 * EPS
    # values that are not finite are skipped
    vals[3] = np.nan
    vals[11] = np.inf
    I2 = integrate_twin(t, vals)
    assert np.isfinite(I2).all() and np.array_equal(I2[2:], I[2:])


def closed_form(table, clim, c, L):
    """The render of the constant field c over a chord of length L."""
    K = table.shape[0]
    s = min(1.0, max(0.0, (c - clim[0]) / (clim[1] - clim[0])))
    f = s * (K - 1)
    j = min(int(math.floor(f)), K - 2)
    row = table[j] + (f - j) * (table[j + 1] - table[j])
    a = -np.expm1(-row[3] * L)
    return np.concatenate([row[:3, None] * a[None, :], a[None, :]]).T


def render_bound(n, table):
    return 16 * (n + 1) * EPS * max(1.0, float(np.abs(table[:, :3]).max()))


def test_twin_renders_a_constant_field_exactly():
    o, d, chord = centre_rays()
    t = rays_twin(CUBE, o, d, 0.13)
    assert np.abs(t.chord - chord).max() <= 8 * EPS * 4 and (t.n > 0).all()
    for c in (0.31, -0.9, 2.0):                    # inside clim, below, above
        got = render_twin(t, np.full(t.pts.shape[0], c), TABLE5, *CLIM)
        want = closed_form(TABLE5, CLIM, c, chord)
        assert (np.abs(got - want) <= render_bound(t.n, TABLE5)[:, None]).all(), c
    # samples without a finite value contribute nothing: the chord shortens by one step each
    vals = np.full(t.pts.shape[0], 0.31)
    vals[t.offsets[:-1]] = np.nan
    got = render_twin(t, vals, TABLE5, *CLIM)
    want = closed_form(TABLE5, CLIM, 0.31, chord - t.h)
    assert (np.abs(got - want) <= render_bound(t.n, TABLE5)[:, None]).all()


def test_twin_misses_and_ranges():
    o = np.array([[-3.0, 0.0, 0.0], [-3.0, 1.5, 0.0], [0.0, 0.0, 0.0], [-3.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    d = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    t = rays_twin(CUBE, o, d, 0.25, 0.0, 3.0)
    assert np.array_equal(t.n, [4, 0, 4, 4, 0])                # cut at t = 3; outside in y; from the centre; ...; away
    assert np.array_equal(t.offsets, [0, 4, 4, 8, 12, 12])
    assert np.array_equal(t.pts[:4, 0], [-0.875, -0.625, -0.375, -0.125])
    assert np.array_equal(t.pts[4:8, 2], [-0.125, -0.375, -0.625, -0.875])
    assert np.array_equal(t.h, [0.25, 0.0, 0.25, 0.25, 0.0])
    # a chord shorter than half a step still gets one sample
    t = rays_twin(CUBE, o[:1], d[:1], 0.25, 0.0, 2.0 + 0.01)
    assert np.array_equal(t.n, [1]) and t.h[0] == (2.0 + 0.01) - 2.0
