"""Frames of a `fem3d` solution: `FigureRenderer` (the figure of `render_figure` for one field after another, everything
that does not depend on the field resident on the device), `animation_timeline` and `render_animation`.

The reference animates a `fem3d` parabolic solution by drawing its default figure once per video frame with the colour
limits and the isosurface levels fixed from the global range of the trajectory (`plot(M, ts, U)` and
`plot(sol::ParabolicSOL, k)`, ext/MultiGridBarrierPyPlotExt/plot3d.jl:310-381), and times the frames through
`_anim_timeline` (MultiGridBarrierPyPlotExt.jl:157-176).  `render_figure` rebuilds everything per call: the located
samples of the volume, the rays, the soup, the hits and the layers all cross the host.  A `FigureRenderer` keeps the
mesh, the rays, the located samples and the tables on the device and chains the same kernels there
(csrc/figure.hip): per frame the field goes in and the image comes out, and the image is bitwise `render_figure`'s.
Nothing here plots or encodes: the frames are plain arrays.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from ._handle import DeviceObject
from .interpolate import _c_f64
from .multigrid import Geometry
from .parabolic import ParabolicSOL
from .raycast import _check_size, _check_transfer, _diagonal, _raycast_plan, camera_rays, clip_box, default_transfer
from .surface import MAX_HITS, REFERENCE_ISOSURFACES, _check_ambient, _check_rays, _clim
from .tensorfem import TensorFEM

MAX_LEVELS = 64         # csrc/figure.hpp FIGURE_MAX_LEVELS
MAX_SLICES = 16         # csrc/figure.hpp FIGURE_MAX_SLICES


def _check_background(who: str, background) -> np.ndarray:
    try:
        b = np.asarray(background, dtype=np.float64)
    except (TypeError, ValueError):
        b = None
    if b is None or b.shape != (3,) or not np.all(np.isfinite(b)):
        raise ValueError(f"{who}: background must be three finite numbers (got {background!r})")
    return b


def _fem3d_plan(geom, who: str):
    """`_raycast_plan` for the one family that has a figure with a volume: `fem3d`."""
    if not isinstance(geom, Geometry):
        raise ValueError(f"{who}: geom must be a Geometry (got {type(geom).__name__})")
    disc = geom.discretization
    if isinstance(disc, TensorFEM) and disc.e != disc.d:
        raise ValueError(f"{who}: fem{disc.d}d embedded in {disc.e} dimensions is not supported (fem3d only)")
    family, name, dim, k, p, N, xnodes, table = _raycast_plan(geom, who)
    if dim != 3:
        raise ValueError(f"{who}: {name} geometries are not supported (the camera is 3-D: fem3d only)")
    return family, name, k, p, N, xnodes, table


class FigureRenderer(DeviceObject):
    """`render_figure(geom, u, eye, target, ...)` for many `u`: the camera, the isosurface levels, the slices, the colour
    limits and the tables are fixed when the renderer is made, and `render(u)` is bitwise what `render_figure` returns
    for the same arguments (the same kernels run on the same inputs; only where the data lives between them differs).

    `isosurfaces` (the level values; `[]` draws none) and `clim = (lo, hi)` are required: a renderer serves a whole
    trajectory, so neither can default to the range of one frame.  `slices`, `volume`, `surface_alpha`, `step`,
    `transfer` and `ambient` are those of `render_figure`.  Only `fem3d` geometries are accepted; `lines=` and `fem2d`
    surfaces in R^3 are not part of the resident path.

    Resident on the device: the mesh, the rays, the levels, the slices' coordinate functions, both colour tables and,
    with `volume=True`, the samples of every ray located once.  Per frame the host sends `u` and receives the image;
    the soup, its grid, the hits and the layers stay on the device, in buffers that grow to the largest frame seen.

    Attributes: `size = (W, H)`, `nrays`, and after a frame `ntriangles` and `npairs` (the soup and its grid's
    (cell, triangle) pairs).  Use it as a context manager or call `close()`.
    """

    _closed_message = "FigureRenderer: the renderer is closed"
    _destroy = "mgbhip_figure_destroy"

    def __init__(self, geom: Geometry, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0, *, isosurfaces,
                 clim, slices=None, volume: bool = True, surface_alpha: float = 1.0, step: Optional[float] = None,
                 transfer=None, ambient: float = 0.3, device_id: int = 0):
        who = "FigureRenderer"
        family, self._name, k, self._p, self._N, xnodes, ctable = _fem3d_plan(geom, who)
        W, H = _check_size(size)
        o, d = camera_rays(eye, target, up, (W, H), fov)
        if clim is None:
            raise ValueError(f"{who}: clim=(lo, hi) is required (the limits are fixed for the renderer's life)")
        lo, hi = _clim(who, clim, np.zeros(0), "u")
        box = clip_box(geom)
        table = default_transfer(_diagonal(box)) if transfer is None else _check_transfer(transfer)
        if not (isinstance(surface_alpha, (int, float, np.integer, np.floating)) and 0.0 <= surface_alpha <= 1.0):
            raise ValueError(f"{who}: surface_alpha must be a number in [0, 1] (got {surface_alpha!r})")
        ambient = _check_ambient(who, ambient)
        if isosurfaces is None:
            raise ValueError(f"{who}: isosurfaces is required (the levels are fixed for the renderer's life; [] draws none)")
        lev = np.asarray(isosurfaces, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(lev)):
            raise ValueError(f"{who}: every entry of isosurfaces must be finite")
        if lev.shape[0] > MAX_LEVELS:
            raise ValueError(f"{who}: isosurfaces has {lev.shape[0]} levels; at most {MAX_LEVELS} are supported")
        planes = []
        for s in ([] if slices is None else slices):
            try:
                axis, coord = s
                coord = float(coord)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: slices must be a list of (axis, coordinate) pairs (got {s!r})") from None
            if isinstance(axis, bool) or not isinstance(axis, (int, np.integer)) or axis not in (0, 1, 2) \
                    or not math.isfinite(coord):
                raise ValueError(f"{who}: a slice needs an axis in 0..2 and a finite coordinate (got {s!r})")
            planes.append((int(axis), coord))
        if len(planes) > MAX_SLICES:
            raise ValueError(f"{who}: slices has {len(planes)} planes; at most {MAX_SLICES} are supported")
        if step is None:
            step = _diagonal(box) / 256.0
        elif not (isinstance(step, (int, float, np.integer, np.floating)) and math.isfinite(step) and step > 0.0):
            raise ValueError(f"{who}: step must be finite and positive (got {step!r})")
        if not isinstance(volume, (bool, np.bool_)):
            raise ValueError(f"{who}: volume must be True or False (got {volume!r})")
        O, Dn = _check_rays(who, o, d)
        surf_table = table.copy()
        surf_table[:, 3] = float(surface_alpha)
        K = 1 if surface_alpha == 1 else 4
        assert K <= MAX_HITS
        self.size = (W, H)
        self.nrays = R = int(O.shape[0])
        self.ntriangles = self.npairs = 0
        self.levels, self.clim, self.slices = lev.copy(), (lo, hi), list(planes)

        from .device import _ptr
        O, Dn, box, xnodes, ctable = _c_f64(O), _c_f64(Dn), _c_f64(box), _c_f64(xnodes), _c_f64(ctable)
        table, surf_table, lev = _c_f64(table), _c_f64(surf_table), _c_f64(lev)
        axes = np.ascontiguousarray([a for a, _ in planes], dtype=np.int32)
        coords = _c_f64(np.array([c for _, c in planes], dtype=np.float64))
        self._create(device_id, "mgbhip_figure_create", family, 3, k, self._p, self._N, _ptr(xnodes), _ptr(ctable), R,
                     _ptr(O), _ptr(Dn), _ptr(box), float(step), 1 if volume else 0, int(lev.shape[0]), _ptr(lev),
                     len(planes), axes.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(coords), int(table.shape[0]),
                     _ptr(table), _ptr(surf_table), lo, hi, ambient, K, invalid_is_value_error=True)

    def _field(self, who: str, u) -> np.ndarray:
        U = np.asarray(u, dtype=np.float64)
        if U.ndim != 1 or U.shape[0] != self._p * self._N:
            raise ValueError(f"{who}: u must be a vector of {self._p * self._N} values for this {self._name} geometry "
                             f"(got shape {U.shape})")
        return _c_f64(U)

    def _counts(self):
        from .device import _check
        t, n = C.c_int64(0), C.c_int64(0)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_figure_counts(self._handle, C.byref(t), C.byref(n)))
        self.ntriangles, self.npairs = int(t.value), int(n.value)

    def render(self, u) -> np.ndarray:
        """`(H, W, 4)` float64: premultiplied colour and alpha of the figure of `u` (`(p*N,)`), row 0 at the top."""
        self._open()
        U = self._field("FigureRenderer.render", u)
        from .device import _check, _ptr
        W, H = self.size
        out = np.empty((H, W, 4))
        _check(self._ctx.lib, self._ctx.lib.mgbhip_figure_render(self._handle, _ptr(U), _ptr(out)))
        self._counts()
        return out

    def render_rgba8(self, u, background=(1, 1, 1)) -> np.ndarray:
        """`(H, W, 4)` uint8: the frame of `render(u)` over `background` (three finite numbers), converted on the device:
        per colour channel `c = C + (1 - alpha) b`, `q = floor(255 min(1, max(0, c)) + 0.5)`, 0 for a `c` that is not
        finite; the fourth byte is the same rule applied to alpha."""
        self._open()
        who = "FigureRenderer.render_rgba8"
        U = self._field(who, u)
        b = _c_f64(_check_background(who, background))
        from .device import _check, _ptr
        W, H = self.size
        out = np.empty((H, W, 4), dtype=np.uint8)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_figure_render_rgba8(self._handle, _ptr(U), _ptr(b),
                                                                      out.ctypes.data_as(C.POINTER(C.c_uint8))))
        self._counts()
        return out


def animation_timeline(ts, frame_time: Optional[float] = None, nframes: Optional[int] = None):
    """`(n_video_frames, frame_index)`: the reference's `_anim_timeline` (MultiGridBarrierPyPlotExt.jl:157-176).

    `ts` are the non-decreasing time stamps of the data frames.  Video frame `j` shows, at the time `min(j frame_time,
    ts[-1] - ts[0])` after `ts[0]`, the latest data frame whose time stamp is not after it; `frame_index[j]` is its
    0-based index, `n_video_frames = max(1, floor((ts[-1] - ts[0]) / frame_time) + 1)`.  `frame_time` defaults to
    `max(0.001, min(diff(ts)))` (0.001 for a single stamp).  `nframes`, when given, must equal `len(ts)`.  A length
    mismatch, an empty or decreasing `ts` and a `frame_time` that is not finite and positive raise `ValueError`.
    """
    who = "animation_timeline"
    t = np.asarray(ts, dtype=np.float64)
    if t.ndim != 1 or t.shape[0] == 0:
        raise ValueError(f"{who}: ts must be a non-empty 1-D array of time stamps (got shape {t.shape})")
    n = int(t.shape[0])
    if nframes is not None and int(nframes) != n:
        raise ValueError(f"{who}: length(ts)={n} must equal number of frames={int(nframes)}")
    if not np.all(np.isfinite(t)):
        raise ValueError(f"{who}: every time stamp must be finite")
    dt = np.diff(t)
    if np.any(dt < 0):
        raise ValueError(f"{who}: ts must be nondecreasing")
    if frame_time is None:
        frame_time = max(0.001, float(dt.min())) if n > 1 else 0.001
    if isinstance(frame_time, bool) or not isinstance(frame_time, (int, float, np.integer, np.floating)) \
            or not (math.isfinite(frame_time) and frame_time > 0.0):
        raise ValueError(f"{who}: frame_time must be finite and positive (got {frame_time!r})")
    frame_time = float(frame_time)
    t0 = t - t[0]
    total = float(t0[-1])
    nvideo = max(1, int(math.floor(total / frame_time)) + 1)
    index = np.zeros(nvideo, dtype=np.int64)
    cur = 0
    for j in range(nvideo):
        tj = min(j * frame_time, total)
        while cur + 1 < n and t0[cur + 1] <= tj:
            cur += 1
        index[j] = cur
    return nvideo, index


def render_animation(geom_or_sol, ts=None, U=None, k: int = 0, frame_time: Optional[float] = None, rgba8: bool = False,
                     background=(1, 1, 1), **figure_kwargs) -> np.ndarray:
    """`(n_video_frames, H, W, 4)`: the frames of the reference's animation of a `fem3d` time series
    (plot3d.jl:310-381), float64 premultiplied colour and alpha, or uint8 over `background` with `rgba8=True`.

    Either `render_animation(geom, ts, U, ...)` with `U` of shape `(p*N, nframes)` (column `j` is the field at `ts[j]`),
    or `render_animation(sol, k=..., ...)` with a `ParabolicSOL`: its geometry, its `ts` and component `k` (0-based)
    of every `sol.u[j]`.  `figure_kwargs` go to `FigureRenderer` (`eye` and `target` are required).  As in the
    reference the colour limits and the levels are fixed over the trajectory: `clim` defaults to the minimum and
    maximum of the finite entries of `U` and `isosurfaces` to `[0.1, 0.3, 0.5, 0.7, 0.9] * (max - min) + min` of that
    range.  The video frames follow `animation_timeline(ts, frame_time)`; each distinct data frame is rendered once
    by one `FigureRenderer` and repeated video frames are copies, so frame `j` is bitwise
    `render_figure(geom, U[:, frame_index[j]], ...)` with the same `clim` and `isosurfaces`.
    """
    who = "render_animation"
    if isinstance(geom_or_sol, ParabolicSOL):
        sol = geom_or_sol
        if ts is not None or U is not None:
            raise ValueError(f"{who}: a ParabolicSOL brings its own ts and U; give k= to pick the component")
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise ValueError(f"{who}: k must be an integer (got {k!r})")
        if len(sol.u) == 0:
            raise ValueError(f"{who}: the ParabolicSOL has no frames")
        ncomp = int(np.asarray(sol.u[0]).shape[1])
        if not 0 <= k < ncomp:
            raise ValueError(f"{who}: k = {k} is outside 0..{ncomp - 1}, the components of this ParabolicSOL")
        geom, ts = sol.geometry, np.asarray(sol.ts, dtype=np.float64)
        U = np.stack([np.asarray(uj, dtype=np.float64)[:, k] for uj in sol.u], axis=1)
    else:
        geom = geom_or_sol
        if ts is None or U is None:
            raise ValueError(f"{who}: give (geom, ts, U) or a ParabolicSOL")
    _, name, _, p, N, _, _ = _fem3d_plan(geom, who)
    U = np.asarray(U, dtype=np.float64)
    if U.ndim != 2 or U.shape[0] != p * N or U.shape[1] == 0:
        raise ValueError(f"{who}: U must be ({p * N}, nframes) for this {name} geometry (got shape {U.shape})")
    try:
        nvideo, index = animation_timeline(ts, frame_time, nframes=U.shape[1])
    except ValueError as e:
        raise ValueError(str(e).replace("animation_timeline:", f"{who}:", 1)) from None
    if not isinstance(rgba8, (bool, np.bool_)):
        raise ValueError(f"{who}: rgba8 must be True or False (got {rgba8!r})")
    bg = _check_background(who, background)
    for name_ in ("eye", "target"):
        if name_ not in figure_kwargs:
            raise ValueError(f"{who}: {name_}= is required (the camera of FigureRenderer)")
    kw = dict(figure_kwargs)
    if kw.get("clim") is None or kw.get("isosurfaces") is None:
        fin = U[np.isfinite(U)]
        if fin.size == 0:
            raise ValueError(f"{who}: U has no finite entry to take the default clim from")
        lo, hi = float(fin.min()), float(fin.max())
        if kw.get("clim") is None:
            if not lo < hi:
                raise ValueError(f"{who}: U is constant ({lo}); give clim=(lo, hi)")
            kw["clim"] = (lo, hi)
        if kw.get("isosurfaces") is None:
            kw["isosurfaces"] = np.array(REFERENCE_ISOSURFACES) * (hi - lo) + lo
    eye, target = kw.pop("eye"), kw.pop("target")
    try:
        fr = FigureRenderer(geom, eye, target, **kw)
    except ValueError as e:
        raise ValueError(str(e).replace("FigureRenderer:", f"{who}:", 1)) from None
    except TypeError as e:
        raise ValueError(f"{who}: {e}") from None
    with fr:
        W, H = fr.size
        frames = np.empty((nvideo, H, W, 4), dtype=np.uint8 if rgba8 else np.float64)
        last = -1
        for j in range(nvideo):
            i = int(index[j])
            if i == last:
                frames[j] = frames[j - 1]
                continue
            col = np.ascontiguousarray(U[:, i])
            frames[j] = fr.render_rgba8(col, bg) if rgba8 else fr.render(col)
            last = i
    return frames
