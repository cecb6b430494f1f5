"""FigureRenderer / render_animation on the device against render_figure, the unchanged host chain of the same stages.

Both sides run the same kernels on the same inputs (the renderer only keeps the data on the device between them), so
every comparison is `np.array_equal`: no tolerance and no margin condition.  One renderer draws four frames in a row
whose soups grow, vanish and shrink (a smooth field, a constant one with no isosurface triangle, |x|^2, the first
again), so that the kept buffers are larger than a frame needs and an empty soup comes between two full ones.  The
reference images are computed once per configuration and frame and shared by the tests (never modified).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import mgb_amd as m
from figure_twin import rgba8_twin
from mgb_amd.figure import FigureRenderer, render_animation
from mgb_amd.raycast import _diagonal, clip_box
from mgb_amd.surface import render_figure
from test_raycast import smooth
from test_surface import sphere_geom

pytestmark = pytest.mark.gpu

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)
GEOMS = {"k1x64": sphere_geom, "k2x8": lambda: m.subdivide(m.fem3d(k=2), 1)}
SIZES = [(32, 24), (5, 3)]                   # 768 rays: three blocks; 15 rays: part of one wave
LEVELS = [-0.35, 0.2, 0.61, 1.1]
CLIM = (-1.0, 3.0)
SLICES = [(0, 0.25), (2, -0.1)]
AMBIENT = 0.25
# FigureRenderer.npairs of the four frames per (geometry, sliced): the (cell, triangle) pairs of the soup's grid, which
# depend on the soup alone.  Results cannot see a changed cell count (it only changes speed); these do.  Recorded from
# the build before the grid builders were merged.  "k1x64" sliced, frame 2 goes through the coarsening loop: 928
# triangles at 4 cells per box give 16^3 cells and 22808 pairs, above 16 * 928 + 4096 = 18944, so the grid is rebuilt
# at 0.5 cells per box (8^3 cells); every other soup keeps its first grid.
NPAIRS = {("k1x64", False): (7291, 0, 12828, 7291), ("k1x64", True): (13894, 1296, 7968, 13894),
          ("k2x8", False): (2153, 0, 3108, 2153), ("k2x8", True): (3990, 400, 5512, 3990)}


@functools.lru_cache(maxsize=None)
def geometry(name):
    return GEOMS[name]()


@functools.lru_cache(maxsize=None)
def fields(name):
    """The four frames: smooth, constant (no isosurface triangle: 0.4 is no level), |x|^2, smooth again."""
    X = geometry(name).xflat
    s = np.ascontiguousarray(smooth(X)[:, 0])
    out = (s, np.full(X.shape[0], 0.4), np.sum(X * X, axis=1), s.copy())
    for a in out:
        a.setflags(write=False)
    return out


def figure_args(name, size, volume, alpha, sliced):
    geom = geometry(name)
    return dict(size=size, isosurfaces=LEVELS, clim=CLIM, slices=SLICES if sliced else None, volume=volume,
                surface_alpha=alpha, step=_diagonal(clip_box(geom)) / 16.0, ambient=AMBIENT)


@functools.lru_cache(maxsize=None)
def reference(name, size, volume, alpha, sliced, frame):
    """render_figure, the parent's unchanged path, for one frame of one configuration."""
    img = render_figure(geometry(name), fields(name)[frame], EYE, TARGET, **figure_args(name, size, volume, alpha, sliced))
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def soup_size(name, frame, sliced):
    geom, u = geometry(name), fields(name)[frame]
    T = m.isocontour(geom, u, LEVELS).points.shape[0]
    if sliced:
        T += sum(m.isocontour(geom, geom.xflat[:, a], [c], carry=u).points.shape[0] for a, c in SLICES)
    return T


@pytest.mark.parametrize("sliced", [False, True], ids=["noslices", "slices"])
@pytest.mark.parametrize("alpha", [1.0, 0.6], ids=["K1", "K4"])
@pytest.mark.parametrize("volume", [True, False], ids=["volume", "surfaces"])
@pytest.mark.parametrize("size", SIZES, ids=["32x24", "5x3"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_frames_are_bitwise_render_figures(name, size, volume, alpha, sliced):
    W, H = size
    frames = []
    with FigureRenderer(geometry(name), EYE, TARGET, **figure_args(name, size, volume, alpha, sliced)) as fr:
        assert fr.nrays == W * H and fr.ntriangles == 0 and fr.npairs == 0
        for j, u in enumerate(fields(name)):
            img = fr.render(u)
            assert img.shape == (H, W, 4) and img.dtype == np.float64
            assert np.array_equal(img, reference(name, size, volume, alpha, sliced, j)), (name, size, volume, alpha, sliced, j)
            T = soup_size(name, j, sliced)
            assert fr.ntriangles == T, "mgbhip_figure_counts reports the frame's soup"
            assert fr.npairs == NPAIRS[name, sliced][j] and (fr.npairs >= T if T else fr.npairs == 0)
            frames.append(img)
    assert soup_size(name, 1, False) == 0, "the constant frame has no isosurface triangle"
    assert soup_size(name, 0, sliced) > 0 and soup_size(name, 2, sliced) != soup_size(name, 0, sliced)
    assert np.array_equal(frames[3], frames[0]), "nothing stale survives in the grown buffers"
    if not volume and not sliced:
        assert not frames[1].any(), "an empty soup without a volume is an empty image"
    assert frames[0][..., 3].max() > 0.0, "the camera sees the figure"


@pytest.mark.parametrize("volume", [True, False], ids=["volume", "surfaces"])
@pytest.mark.parametrize("name", sorted(GEOMS))
def test_rgba8_is_the_twin_of_render(name, volume):
    size, alpha, sliced = (32, 24), 0.6, True
    with FigureRenderer(geometry(name), EYE, TARGET, **figure_args(name, size, volume, alpha, sliced)) as fr:
        for j in (0, 1, 2):
            img = reference(name, size, volume, alpha, sliced, j)
            # the third background is outside [0, 1]: both ends of the clamp are taken on the device
            for bg in ((1.0, 1.0, 1.0), (0.1, 0.45, 0.8), (2.0, -1.0, 0.5)):
                q = fr.render_rgba8(fields(name)[j], bg)
                assert q.shape == (24, 32, 4) and q.dtype == np.uint8
                assert np.array_equal(q, rgba8_twin(img, bg)), (name, volume, j, bg)
        white = fr.render_rgba8(fields(name)[0])
        assert np.array_equal(white, rgba8_twin(reference(name, size, volume, alpha, sliced, 0), (1.0, 1.0, 1.0)))
        assert len(np.unique(white[..., :3])) > 8, "the bytes hold a picture, not a flat colour"


def animation_case():
    name, size = "k1x64", (32, 24)
    f = fields(name)
    U = np.stack([f[0], f[2], 0.5 * f[0] + 0.5 * f[2]], axis=1)
    lo, hi = float(U.min()), float(U.max())
    lev = np.array([0.1, 0.3, 0.5, 0.7, 0.9]) * (hi - lo) + lo
    kw = dict(size=size, step=_diagonal(clip_box(geometry(name))) / 16.0, slices=[(1, 0.3)])
    return name, size, U, (lo, hi), lev, kw


def test_render_animation_frames_are_render_figures():
    name, (W, H), U, clim, lev, kw = animation_case()
    geom = geometry(name)
    ts = [0.0, 0.5, 2.0]
    frames = render_animation(geom, ts, U, frame_time=0.5, eye=EYE, target=TARGET, **kw)
    assert frames.shape == (5, H, W, 4) and frames.dtype == np.float64
    assert np.array_equal(frames[1], frames[2]) and np.array_equal(frames[2], frames[3])
    refs = [render_figure(geom, U[:, j], EYE, TARGET, isosurfaces=lev, clim=clim, **kw) for j in range(3)]
    for j, i in enumerate([0, 1, 1, 1, 2]):
        assert np.array_equal(frames[j], refs[i]), (j, i)
    assert not np.array_equal(refs[0], refs[1]) and not np.array_equal(refs[1], refs[2])
    # the same trajectory as component 1 of a hand-made ParabolicSOL
    other = np.cos(geom.xflat[:, 0])
    sol = m.ParabolicSOL(geometry=geom, ts=np.array(ts), u=[np.stack([other, U[:, j]], axis=1) for j in range(3)])
    again = render_animation(sol, k=1, frame_time=0.5, eye=EYE, target=TARGET, **kw)
    assert np.array_equal(again, frames)
    # bytes: the twin of every frame
    q = render_animation(sol, k=1, frame_time=0.5, rgba8=True, background=(0.2, 0.2, 0.2), eye=EYE, target=TARGET, **kw)
    assert q.shape == (5, H, W, 4) and q.dtype == np.uint8
    assert np.array_equal(q, rgba8_twin(frames, (0.2, 0.2, 0.2)))


def test_two_renderers_alive_at_once():
    name = "k2x8"
    a_cfg, b_cfg = ((32, 24), True, 0.6, True), ((5, 3), False, 1.0, False)
    with FigureRenderer(geometry(name), EYE, TARGET, **figure_args(name, *a_cfg)) as a, \
            FigureRenderer(geometry(name), EYE, TARGET, **figure_args(name, *b_cfg)) as b:
        for j in (0, 2, 1, 0):
            ia = a.render(fields(name)[j])
            ib = b.render(fields(name)[(j + 1) % 3])
            assert np.array_equal(ia, reference(name, *a_cfg, j))
            assert np.array_equal(ib, reference(name, *b_cfg, (j + 1) % 3))
        b.close()
        assert np.array_equal(a.render(fields(name)[2]), reference(name, *a_cfg, 2)), "closing one leaves the other"


def test_closed_renderer_and_bad_fields_raise():
    name = "k1x64"
    fr = FigureRenderer(geometry(name), EYE, TARGET, **figure_args(name, (5, 3), False, 1.0, False))
    with pytest.raises(ValueError, match="u must be a vector of"):
        fr.render(fields(name)[0][:-1])
    with pytest.raises(ValueError, match="background must be three finite numbers"):
        fr.render_rgba8(fields(name)[0], background=(1, 1))
    fr.close()
    fr.close()
    assert fr.closed
    with pytest.raises(ValueError, match="the renderer is closed"):
        fr.render(fields(name)[0])
    with pytest.raises(ValueError, match="the renderer is closed"):
        fr.render_rgba8(fields(name)[0])


def test_c_abi_refusals():
    from mgb_amd import device
    from mgb_amd.interpolate import _plan
    from mgb_amd.raycast import camera_rays, default_transfer, normalize
    geom = geometry("k1x64")
    family, _, d, k, p, N, x, table = _plan(geom)
    o, dirs = camera_rays(EYE, TARGET, size=(5, 3))
    dn = normalize(dirs)
    box = clip_box(geom)
    vt = default_transfer(_diagonal(box))
    st = vt.copy()
    st[:, 3] = 1.0
    lev = np.array(LEVELS)
    ptr = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (x, table, o, dn, box, lev, vt, st)]
    xs, ts_, os_, ds, bs, ls, vts, sts = (a.ctypes.data_as(C.POINTER(C.c_double)) for a in keep)
    coords = np.array([0.25])
    ctx = device.HipContext(0)
    lib = ctx.lib

    def create(K=1, nlevels=len(LEVELS), axis=0, nslices=1):
        axes = np.array([axis], dtype=np.int32)
        h = C.c_void_p()
        rc = lib.mgbhip_figure_create(ctx.handle, family, d, k, p, N, xs, ts_, 15, os_, ds, bs, 0.2, 1, nlevels, ls, nslices,
                                      axes.ctypes.data_as(C.POINTER(C.c_int32)), ptr(coords), vt.shape[0], vts, sts,
                                      CLIM[0], CLIM[1], AMBIENT, K, C.byref(h))
        return rc, h, lib.mgbhip_last_error().decode()

    try:
        for kwargs, message in ((dict(K=0), "K must be 1..8"), (dict(K=9), "K must be 1..8"),
                                (dict(nlevels=-1), "nlevels must be 0..64"), (dict(nlevels=65), "nlevels must be 0..64"),
                                (dict(axis=3), "axis in 0..2"), (dict(axis=-1), "axis in 0..2"),
                                (dict(nslices=17), "nslices must be 0..16")):
            rc, h, err = create(**kwargs)
            assert rc == device.ERR_INVALID and message in err and not h.value, (kwargs, rc, err)
        u = np.zeros(p * N)
        out = np.zeros((15, 4))
        q = np.zeros((15, 4), dtype=np.uint8)
        bg = np.ones(3)
        assert lib.mgbhip_figure_render(None, ptr(u), ptr(out)) == device.ERR_INVALID
        assert "null figure" in lib.mgbhip_last_error().decode()
        assert lib.mgbhip_figure_render_rgba8(None, ptr(u), ptr(bg), q.ctypes.data_as(C.POINTER(C.c_uint8))) == device.ERR_INVALID
        n = C.c_int64(7)
        assert lib.mgbhip_figure_counts(None, C.byref(n), None) == device.ERR_INVALID and n.value == 7
        assert lib.mgbhip_figure_destroy(None) == 0, "NULL is a no-op"
        # a good handle: NULL arguments are refused, a frame works, counts may skip either output
        rc, h, err = create()
        assert rc == 0, err
        try:
            assert lib.mgbhip_figure_render(h, None, ptr(out)) == device.ERR_INVALID
            assert lib.mgbhip_figure_render(h, ptr(u), None) == device.ERR_INVALID
            assert lib.mgbhip_figure_render_rgba8(h, ptr(u), None, q.ctypes.data_as(C.POINTER(C.c_uint8))) == device.ERR_INVALID
            assert lib.mgbhip_figure_render(h, ptr(fields("k1x64")[0]), ptr(out)) == 0, lib.mgbhip_last_error()
            assert lib.mgbhip_figure_counts(h, C.byref(n), None) == 0 and n.value > 0
            assert lib.mgbhip_figure_counts(h, None, C.byref(n)) == 0 and n.value > 0
        finally:
            assert lib.mgbhip_figure_destroy(h) == 0
    finally:
        ctx.close()
