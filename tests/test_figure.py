"""FigureRenderer / animation_timeline / render_animation without a device: the timeline against hand-computed cases,
the NumPy twin of the byte conversion against hand values, and every argument refusal, which must come before any
device work (this file runs where there is no GPU: a refusal that reached the device layer would not be a ValueError)."""
import numpy as np
import pytest

import mgb_amd as m
from figure_twin import rgba8_twin
from manifold_twin import cubed_sphere
from mgb_amd.figure import FigureRenderer, animation_timeline, render_animation

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------
# the timeline
# ---------------------------------------------------------------------------------------------------------------

def test_timeline_default_frame_time_shows_every_frame_once():
    n, idx = animation_timeline([0.0, 1.0, 2.0])
    assert n == 3 and idx.tolist() == [0, 1, 2] and np.issubdtype(idx.dtype, np.integer)


def test_timeline_uneven_stamps_repeat_the_latest_frame():
    # video times 0, 0.5, 1, 1.5, 2: frame 1 (t = 0.5) is the latest until t = 2
    n, idx = animation_timeline([0.0, 0.5, 2.0], frame_time=0.5)
    assert n == 5 and idx.tolist() == [0, 1, 1, 1, 2]
    # the origin of ts does not matter
    n, idx = animation_timeline([10.0, 10.5, 12.0], frame_time=0.5)
    assert n == 5 and idx.tolist() == [0, 1, 1, 1, 2]


def test_timeline_repeated_stamps_show_the_last_of_them():
    # stamps 0, 0, 1, 1 at video times 0, 0.5, 1: the later of two equal stamps wins, as in the reference's while loop
    n, idx = animation_timeline([0.0, 0.0, 1.0, 1.0], frame_time=0.5)
    assert n == 3 and idx.tolist() == [1, 1, 3]
    # all stamps equal: one video frame, the last data frame
    n, idx = animation_timeline([3.0, 3.0, 3.0], frame_time=0.25)
    assert n == 1 and idx.tolist() == [2]
    # the default frame time has the floor 0.001 when two stamps coincide: 0.002 / 0.001 + 1 frames
    n, idx = animation_timeline([0.0, 0.0, 0.002])
    assert n == 3 and idx.tolist() == [1, 1, 2]


def test_timeline_single_stamp_and_coarse_frame_time():
    n, idx = animation_timeline([0.7])
    assert n == 1 and idx.tolist() == [0]
    # a frame time longer than the series: the first frame alone
    n, idx = animation_timeline([0.0, 1.0, 2.0], frame_time=5.0)
    assert n == 1 and idx.tolist() == [0]
    # a frame time that skips data frames
    n, idx = animation_timeline([0.0, 1.0, 2.0, 3.0, 4.0], frame_time=2.0)
    assert n == 3 and idx.tolist() == [0, 2, 4]


def test_timeline_refusals():
    with pytest.raises(ValueError, match="must equal number of frames"):
        animation_timeline([0.0, 1.0, 2.0], nframes=2)
    with pytest.raises(ValueError, match="nondecreasing"):
        animation_timeline([0.0, 2.0, 1.0])
    with pytest.raises(ValueError, match="non-empty"):
        animation_timeline([])
    with pytest.raises(ValueError, match="finite"):
        animation_timeline([0.0, np.nan])
    for bad in (0.0, -1.0, np.inf, np.nan, "1", True):
        with pytest.raises(ValueError, match="frame_time"):
            animation_timeline([0.0, 1.0], frame_time=bad)


# ---------------------------------------------------------------------------------------------------------------
# the byte conversion
# ---------------------------------------------------------------------------------------------------------------

def px(r, g, b, a):
    return np.array([[r, g, b, a]], dtype=np.float64)


def test_rgba8_twin_hand_values():
    black = (0.0, 0.0, 0.0)
    assert rgba8_twin(px(0.0, 1.0, 0.5, 1.0), black).tolist() == [[0, 255, 128, 255]]
    # a half step: 255 c + 0.5 is a whole number at c = 0.5 (127.5 + 0.5); one ulp below rounds down, one above stays
    under, over = np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)
    assert rgba8_twin(px(under, 0.5, over, 1.0), black).tolist() == [[127, 128, 128, 255]]
    # 1 / 510 is the first half step: 255 / 510 + 0.5 = 1
    assert rgba8_twin(px(0.0019, 0.002, 0.0, 1.0), black).tolist() == [[0, 1, 0, 255]]
    # clamped below and above; alpha too
    assert rgba8_twin(px(-0.3, 1.7, -0.0, 1.0), black).tolist() == [[0, 255, 0, 255]]
    assert rgba8_twin(px(0.0, 0.0, 0.0, 2.5), black)[0, 3] == 255 and rgba8_twin(px(0.0, 0.0, 0.0, -1.0), black)[0, 3] == 0
    # not finite: 0, per channel
    assert rgba8_twin(px(np.nan, np.inf, -np.inf, 1.0), black).tolist() == [[0, 0, 0, 255]]
    assert rgba8_twin(px(0.25, 0.25, 0.25, np.nan), black).tolist() == [[0, 0, 0, 0]]      # c = C + NaN b
    assert rgba8_twin(np.zeros((2, 3, 4))).dtype == np.uint8 and rgba8_twin(np.zeros((2, 3, 4))).shape == (2, 3, 4)


def test_rgba8_twin_background_shows_through():
    # alpha 0: the background alone; 0.2 * 255 = 51, 0.4 * 255 = 102, 1.0 -> 255
    assert rgba8_twin(px(0.0, 0.0, 0.0, 0.0), (0.2, 0.4, 1.0)).tolist() == [[51, 102, 255, 0]]
    # alpha 0.5 over white: c = C + 0.5; premultiplied (0.25, 0, 0.5) -> 0.75, 0.5, 1.0 -> 191, 128, 255; alpha -> 128
    assert rgba8_twin(px(0.25, 0.0, 0.5, 0.5)).tolist() == [[191, 128, 255, 128]]
    # opaque: the background does not matter
    assert np.array_equal(rgba8_twin(px(0.1, 0.2, 0.3, 1.0), (1, 1, 1)), rgba8_twin(px(0.1, 0.2, 0.3, 1.0), (0, 0, 0)))


# ---------------------------------------------------------------------------------------------------------------
# refusals, before any device work
# ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def geom():
    return m.fem3d(k=1)


OK = dict(isosurfaces=[0.5], clim=(0.0, 1.0), size=(8, 6))

BAD_RENDERER = [
    (dict(size=(8,)), "size must be"),
    (dict(size=(0, 6)), "size entries"),
    (dict(fov=180.0), "fov must be"),
    (dict(up=(2.7, -3.1, 1.9)), "up is parallel"),
    (dict(clim=None), "clim=\\(lo, hi\\) is required"),
    (dict(clim=(1.0, 1.0)), "FigureRenderer: clim must be finite with lo < hi"),
    (dict(clim=(0.0,)), "FigureRenderer: clim must be \\(lo, hi\\)"),
    (dict(transfer=np.zeros((1, 4))), "transfer must be"),
    (dict(transfer=np.full((4, 4), -1.0)), "sigma must be >= 0"),
    (dict(surface_alpha=1.5), "FigureRenderer: surface_alpha must be a number in \\[0, 1\\]"),
    (dict(surface_alpha="1"), "FigureRenderer: surface_alpha"),
    (dict(ambient=-0.1), "FigureRenderer: ambient must be a number in \\[0, 1\\]"),
    (dict(isosurfaces=None), "isosurfaces is required"),
    (dict(isosurfaces=[0.1, np.nan]), "FigureRenderer: every entry of isosurfaces must be finite"),
    (dict(isosurfaces=np.linspace(0.0, 1.0, 65)), "at most 64"),
    (dict(slices=[0.25]), "FigureRenderer: slices must be a list of \\(axis, coordinate\\) pairs"),
    (dict(slices=[(3, 0.25)]), "FigureRenderer: a slice needs an axis in 0..2"),
    (dict(slices=[(True, 0.25)]), "FigureRenderer: a slice needs an axis in 0..2"),
    (dict(slices=[(0, np.inf)]), "FigureRenderer: a slice needs an axis in 0..2 and a finite coordinate"),
    (dict(slices=[(0, 0.01 * i) for i in range(17)]), "at most 16"),
    (dict(step=0.0), "FigureRenderer: step must be finite and positive"),
    (dict(step="x"), "FigureRenderer: step must be finite and positive"),
    (dict(volume=None), "volume must be True or False"),
]


@pytest.mark.parametrize("change,message", BAD_RENDERER, ids=[f"{i}-{sorted(c)[0]}" for i, (c, _) in enumerate(BAD_RENDERER)])
def test_renderer_refuses_before_device_work(geom, change, message):
    with pytest.raises(ValueError, match=message):
        FigureRenderer(geom, EYE, TARGET, **{**OK, **change})


def test_renderer_refuses_cameras_and_geometries(geom):
    with pytest.raises(ValueError, match="eye and target coincide"):
        FigureRenderer(geom, EYE, EYE, **OK)
    with pytest.raises(ValueError, match="eye must be three finite numbers"):
        FigureRenderer(geom, (0.0, np.nan, 1.0), TARGET, **OK)
    with pytest.raises(TypeError):
        FigureRenderer(geom, EYE, TARGET, size=(8, 6))                # isosurfaces and clim are required keywords
    for other in (m.fem2d(k=1), m.fem1d(nodes=np.linspace(-1, 1, 3)), m.fem2d_P1(), m.spectral1d(n=4)):
        with pytest.raises(ValueError, match="FigureRenderer: .*(fem3d only|not supported)"):
            FigureRenderer(other, EYE, TARGET, **OK)
    with pytest.raises(ValueError, match="FigureRenderer: .*fem3d only"):
        FigureRenderer(m.fem2d(k=1, K=cubed_sphere(1, 1), ambient=3), EYE, TARGET, **OK)
    with pytest.raises(ValueError, match="geom must be a Geometry"):
        FigureRenderer("mesh", EYE, TARGET, **OK)


def test_animation_refuses_before_device_work(geom):
    n = geom.xflat.shape[0]
    U = np.linspace(0.0, 1.0, 3 * n).reshape(n, 3)
    ts = [0.0, 0.5, 2.0]
    cam = dict(eye=EYE, target=TARGET, size=(8, 6))
    bad = [
        (lambda: render_animation(geom, **cam), "give \\(geom, ts, U\\) or a ParabolicSOL"),
        (lambda: render_animation(geom, ts, U[:-1], **cam), "U must be"),
        (lambda: render_animation(geom, ts, U[:, 0], **cam), "U must be"),
        (lambda: render_animation(geom, ts, U[:, :0], **cam), "U must be"),
        (lambda: render_animation(geom, ts[:2], U, **cam), "render_animation: length\\(ts\\)=2 must equal number of frames=3"),
        (lambda: render_animation(geom, [0.0, 2.0, 1.0], U, **cam), "render_animation: ts must be nondecreasing"),
        (lambda: render_animation(geom, ts, U, frame_time=0.0, **cam), "render_animation: frame_time"),
        (lambda: render_animation(geom, ts, U, rgba8=1, **cam), "rgba8 must be True or False"),
        (lambda: render_animation(geom, ts, U, background=(1, 1), **cam), "background must be three finite numbers"),
        (lambda: render_animation(geom, ts, U, background=(1, np.nan, 1), **cam), "background must be three finite"),
        (lambda: render_animation(geom, ts, U, target=TARGET), "eye= is required"),
        (lambda: render_animation(geom, ts, U, eye=EYE), "target= is required"),
        (lambda: render_animation(geom, ts, np.full_like(U, 0.3), **cam), "U is constant"),
        (lambda: render_animation(geom, ts, np.full_like(U, np.nan), **cam), "no finite entry"),
        (lambda: render_animation(geom, ts, U, slices=[(5, 0.0)], **cam), "render_animation: a slice needs an axis"),
        (lambda: render_animation(geom, ts, U, lines=[], **cam), "render_animation: .*lines"),
        (lambda: render_animation(m.fem2d(k=1), ts, U, **cam), "render_animation: .*fem3d only"),
    ]
    for call, message in bad:
        with pytest.raises(ValueError, match=message):
            call()


def test_animation_refuses_a_bad_parabolic_sol(geom):
    n = geom.xflat.shape[0]
    sol = m.ParabolicSOL(geometry=geom, ts=np.array([0.0, 1.0]), u=[np.zeros((n, 2)), np.ones((n, 2))])
    cam = dict(eye=EYE, target=TARGET, size=(8, 6))
    with pytest.raises(ValueError, match="brings its own ts and U"):
        render_animation(sol, [0.0, 1.0], **cam)
    with pytest.raises(ValueError, match="k = 2 is outside 0..1"):
        render_animation(sol, k=2, **cam)
    with pytest.raises(ValueError, match="k must be an integer"):
        render_animation(sol, k=0.0, **cam)
    with pytest.raises(ValueError, match="has no frames"):
        render_animation(m.ParabolicSOL(geometry=geom, ts=np.zeros(0), u=[]), **cam)
    with pytest.raises(ValueError, match="must equal number of frames"):
        render_animation(m.ParabolicSOL(geometry=geom, ts=np.array([0.0]), u=sol.u), **cam)
