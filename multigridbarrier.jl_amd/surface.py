"""Rays against surfaces: `TriangleCaster` (nearest hits of rays with a triangle soup and their shading),
`render_surfaces(contours, eye, target)` and `render_figure(geom, u, eye, target)`.

The reference's picture of a solution on a `fem2d` surface in R^3 cuts every quad into linear cells and draws them
coloured by the solution (ext/MultiGridBarrierPyPlotExt/plot3d.jl:182-256).  `tessellate()` gives those cells as a
triangle soup; `render_surfaces` takes it like a 3-D `Contour`, and `render_figure` on such a geometry traces and shades
it once.

The reference's default picture of a `fem3d` solution draws a volume render, five isosurfaces and optional slices into
one image (ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-149, PyVista on the CPU).  `isocontour()` gives the isosurfaces and
slices as a triangle soup and `RayCaster` the volume render; this module turns the soup into pixels on the device
(csrc/surface.hip) and puts it into the volume's front-to-back compositing at the right depth
(`RayCaster.render(..., layers=...)`).  The host only checks arguments (before any device work), normalises the
directions and concatenates soups.  Nothing here plots or writes image files: the result is a plain array.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._handle import DeviceObject
from .contour import Contour, Tessellation, isocontour, tessellate
from .interpolate import _c_f64
from .multigrid import Geometry
from .tensorfem import TensorFEM
from .raycast import (RayCaster, _check_clim, _check_size, _check_transfer, _diagonal, _raycast_plan, camera_rays, clip_box,
                      default_transfer, normalize)

MAX_HITS = 8            # csrc/surface.hpp SURFACE_MAX_HITS
REFERENCE_ISOSURFACES = (0.1, 0.3, 0.5, 0.7, 0.9)     # plot3d.jl: fractions of the range of u


@dataclass
class Hits:
    """The `K` nearest hits of `R` rays, nearest first; a missing entry is `t = inf`, `triangle = -1`, `u = v = NaN`."""
    t: np.ndarray            # (R, K) float64: the ray parameter (arc length)
    triangle: np.ndarray     # (R, K) int32
    u: np.ndarray            # (R, K) float64: the hit point is (1 - u - v) v0 + u v1 + v v2
    v: np.ndarray            # (R, K) float64


def _check_rays(who: str, o, d):
    O, D = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    if O.ndim == 1 and D.ndim == 1:
        O, D = O.reshape(1, -1), D.reshape(1, -1)
    if O.ndim != 2 or O.shape[1] != 3 or D.shape != O.shape:
        raise ValueError(f"{who}: o and d must both be (R, 3) (got shapes {O.shape} and {D.shape})")
    if not np.all(np.isfinite(O)):
        raise ValueError(f"{who}: every ray origin o must be finite")
    if not np.all(np.isfinite(D)):
        raise ValueError(f"{who}: every ray direction d must be finite")
    if np.any(np.all(D == 0.0, axis=1)):
        raise ValueError(f"{who}: a ray direction d is zero")
    Dn = normalize(D)
    if not np.all(np.abs(np.sum(Dn * Dn, axis=1) - 1.0) <= 1e-12):      # also false for NaN
        raise ValueError(f"{who}: a ray direction d is too long or too short to normalise (sum d*d overflows or vanishes)")
    return O, Dn


def _check_max_hits(who: str, max_hits) -> int:
    if isinstance(max_hits, bool) or not isinstance(max_hits, (int, np.integer)) or not 1 <= max_hits <= MAX_HITS:
        raise ValueError(f"{who}: max_hits must be an integer in 1..{MAX_HITS} (got {max_hits!r})")
    return int(max_hits)


def _check_ambient(who: str, ambient) -> float:
    if not (isinstance(ambient, (int, float, np.integer, np.floating)) and 0.0 <= ambient <= 1.0):
        raise ValueError(f"{who}: ambient must be a number in [0, 1] (got {ambient!r})")
    return float(ambient)


def _check_table(who: str, transfer) -> np.ndarray:
    T = np.asarray(transfer, dtype=np.float64)
    if T.ndim != 2 or T.shape[1] != 4 or T.shape[0] < 2:
        raise ValueError(f"{who}: transfer must be (K, 4) with K >= 2 (got shape {T.shape})")
    if not np.all(np.isfinite(T)):
        raise ValueError(f"{who}: every transfer entry must be finite")
    return T


def _clim(who: str, clim, data: np.ndarray, name: str):
    """`raycast._check_clim` with the errors naming `who` and the argument the default is taken from."""
    try:
        return _check_clim(clim, data)
    except ValueError as e:
        raise ValueError(str(e).replace("RayCaster.render: u ", f"{who}: {name} ").replace("RayCaster.render", who)) from None


def default_surface_table(K: int = 256) -> np.ndarray:
    """The `(K, 4)` table `shade` uses when `transfer` is None: the grey ramp of `default_transfer` with its fourth
    column replaced by 1 (opaque)."""
    T = default_transfer(1.0, K)
    T[:, 3] = 1.0
    return T


def composite_layers(layers: np.ndarray) -> np.ndarray:
    """`(R, 4)`: the layers `(R, K, 4)` of each ray composited front to back from `T = 1, C = 0` by `C += T layer_rgb`,
    `T *= 1 - alpha`; the result is `(C, 1 - T)`.  A sum of at most eight terms per ray, formed on the host."""
    L = np.asarray(layers, dtype=np.float64)
    T = np.ones(L.shape[0])
    Cc = np.zeros((L.shape[0], 3))
    for k in range(L.shape[1]):
        Cc = Cc + T[:, None] * L[:, k, :3]
        T = T * (1.0 - L[:, k, 3])
    return np.concatenate([Cc, (1.0 - T)[:, None]], axis=1)


def _trace_arguments(who: str, o, d, t_min, t_max, max_hits, npar: int):
    """What both casters' `trace` check and allocate: the rays, the window, `K`, and the all-miss hit arrays `t`, index
    and `npar` parameter arrays (`(R, K)` each)."""
    O, Dn = _check_rays(who, o, d)
    try:
        t_min, t_max = float(t_min), float(t_max)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: t_min and t_max must be numbers") from None
    if not math.isfinite(t_min):
        raise ValueError(f"{who}: t_min must be finite (got {t_min})")
    if not t_max > t_min:
        raise ValueError(f"{who}: t_max must be greater than t_min (got t_min = {t_min}, t_max = {t_max})")
    K = _check_max_hits(who, max_hits)
    shape = (int(O.shape[0]), K)
    return (O, Dn, t_min, t_max, K, np.full(shape, np.inf), np.full(shape, -1, dtype=np.int32),
            [np.full(shape, np.nan) for _ in range(npar)])


def _check_hits(who: str, R: int, n: int, rays: str, field: str, index, **others):
    """The index array `hits.<field>` of a `shade` call (`(R, K)`, entries in -1..n-1) and the float arrays
    `hits.<name>` of `others`, which must have its shape."""
    idx = np.asarray(index)
    if idx.ndim != 2 or idx.shape[0] != R or not 1 <= idx.shape[1] <= MAX_HITS:
        raise ValueError(f"{who}: hits hold {idx.shape} entries for {R} {rays}")
    arrays = [np.asarray(a, dtype=np.float64) for a in others.values()]
    if any(a.shape != idx.shape for a in arrays):
        names = " and ".join(f"hits.{name}" for name in others)
        raise ValueError(f"{who}: {names} must have the shape of hits.{field} {idx.shape}")
    if idx.size and (idx.min() < -1 or idx.max() >= n):
        raise ValueError(f"{who}: hits.{field} has an index outside -1..{n - 1}")
    return idx, arrays


def _check_colouring(who: str, values, shape, transfer, clim, ambient):
    """The vertex values (of `shape`), the colour table, the colour limits and the ambient term of a `shade` call."""
    V = np.asarray(values, dtype=np.float64)
    if V.shape != shape:
        raise ValueError(f"{who}: values must be ({shape[0]}, {shape[1]}) (got shape {V.shape})")
    T = default_surface_table() if transfer is None else _check_table(who, transfer)
    if clim is None and shape[0] == 0:
        clim = (0.0, 1.0)                    # nothing to colour
    lo, hi = _clim(who, clim, V, "values")
    return V, T, lo, hi, _check_ambient(who, ambient)


class TriangleCaster(DeviceObject):
    """A triangle soup `points` (`(T, 3, 3)`: triangle, vertex, coordinate; finite) sorted once into a uniform grid of
    cells on the device, for tracing many bundles of rays against it.  `T = 0` is allowed: every ray misses and no
    device work is done.

    The triangle test (the same on the device and in the NumPy restatement the tests compare it with,
    tests/surface_twin.py), for the ray `o + t dn` with `dn = d / sqrt(sum d*d)` and the vertices `v0, v1, v2`, in IEEE
    double without fused multiply-adds, with `(a x b)[0] = a1*b2 - a2*b1` (cyclically) and `a . b = (a0*b0 + a1*b1) + a2*b2`:

        e1 = v1 - v0;  e2 = v2 - v0;  p = dn x e2;  det = e1 . p
        s = o - v0;  u = (s . p) / det;  q = s x e1;  v = (dn . q) / det;  t = (e2 . q) / det

    The triangle is hit iff `det` is finite and non-zero, `u >= 0`, `v >= 0`, `u + v <= 1` and `t_min <= t <= t_max`;
    both sides are hit.  A ray keeps its `max_hits` nearest hits in the order of `(t, triangle index)`.  Which
    triangles a ray is tested against is decided by the grid (a 3-D DDA from the ray's entry into the grid box); what
    it hits is not.

    Use it as a context manager or call `close()`.
    """

    _closed_message = "TriangleCaster: the caster is closed"
    _destroy = "mgbhip_surface_destroy"

    def __init__(self, points, device_id: int = 0):
        P = np.asarray(points, dtype=np.float64)
        if P.ndim != 3 or P.shape[1:] != (3, 3):
            raise ValueError(f"TriangleCaster: points must be (T, 3, 3) (got shape {P.shape})")
        if not np.all(np.isfinite(P)):
            raise ValueError("TriangleCaster: every entry of points must be finite")
        self.ntriangles = T = int(P.shape[0])
        if T:
            from .device import _ptr
            self._create(device_id, "mgbhip_surface_create", T, _ptr(_c_f64(P)))

    def trace(self, o, d, t_min: float = 0.0, t_max: float = np.inf, max_hits: int = 1) -> Hits:
        """The `max_hits` (1..8) nearest hits of every ray `o + t d` (`(R, 3)` each; one ray may be given as `(3,)`) with
        `t_min <= t <= t_max`; `t` is arc length."""
        self._open()
        O, Dn, t_min, t_max, K, t, tri, (u, v) = _trace_arguments("TriangleCaster.trace", o, d, t_min, t_max, max_hits, 2)
        R = int(O.shape[0])
        if R and self.ntriangles:
            from .device import _check, _ptr
            O, Dn = _c_f64(O), _c_f64(Dn)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_surface_trace(
                self._handle, R, _ptr(O), _ptr(Dn), t_min, t_max, K, _ptr(t), tri.ctypes.data_as(C.POINTER(C.c_int32)),
                _ptr(u), _ptr(v)))
        return Hits(t, tri, u, v)

    def shade(self, hits: Hits, d, values, transfer=None, clim=None, ambient: float = 0.3) -> np.ndarray:
        """`(R, K, 4)` float64: premultiplied colour and alpha of every hit.

        `d` are the directions the hits were traced with, `values` is `(T, 3)`: a value per triangle vertex.  The carried
        value of a hit is `c = ((1 - u - v) c0 + u c1) + v c2`; its row of `transfer` (`(K, 4)`: `r, g, b, alpha`; the
        default is `default_surface_table()`) is found as `RayCaster.render` finds it, between `clim = (lo, hi)` (the
        default is the minimum and maximum of the finite `values`).  With `n = e1 x e2`, `nn = n / sqrt(n . n)` and
        `shade = ambient + (1 - ambient) |nn . dn|`, the layer is `alpha shade (r, g, b)` and `alpha = min(1, max(0,
        row[3]))`.  A missing hit or a non-finite `c` gives a zero layer.
        """
        self._open()
        who = "TriangleCaster.shade"
        if not isinstance(hits, Hits):
            raise ValueError(f"{who}: hits must be what trace() returned (got {type(hits).__name__})")
        _, Dn = _check_rays(who, np.zeros_like(np.asarray(d, dtype=np.float64)), d)
        R = int(Dn.shape[0])
        tri, (hu, hv) = _check_hits(who, R, self.ntriangles, "directions d", "triangle", hits.triangle, u=hits.u, v=hits.v)
        K = int(tri.shape[1])
        V, T, lo, hi, ambient = _check_colouring(who, values, (self.ntriangles, 3), transfer, clim, ambient)
        layer = np.zeros((R, K, 4))
        if R and self.ntriangles:
            from .device import _check, _ptr
            Dn, V, T, hu, hv = _c_f64(Dn), _c_f64(V), _c_f64(T), _c_f64(hu), _c_f64(hv)
            tri = np.ascontiguousarray(tri, dtype=np.int32)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_surface_shade(
                self._handle, R, K, _ptr(Dn), tri.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(hu), _ptr(hv), _ptr(V),
                int(T.shape[0]), _ptr(T), lo, hi, ambient, _ptr(layer)))
        return layer


def _soup(who: str, contours, values, levels):
    """The concatenated triangles `(T, 3, 3)` and vertex values `(T, 3)` of one `Contour` or `Tessellation` (of a
    surface in R^3) or a list of them."""
    single = isinstance(contours, (Contour, Tessellation))
    cs = [contours] if single else list(contours)
    for c in cs:
        if isinstance(c, Tessellation):
            if c.points.ndim != 3 or c.points.shape[1:] != (3, 3):
                raise ValueError(f"{who}: a Tessellation must be of a surface in R^3, (T, 3, 3) (got points of shape "
                                 f"{c.points.shape}: the triangles of a flat 2-D mesh have e = 2 coordinates)")
            continue
        if not isinstance(c, Contour):
            raise ValueError(f"{who}: contours must be a Contour or a list of them (got {type(c).__name__})")
        if c.points.ndim != 3 or c.points.shape[1:] != (3, 3):
            raise ValueError(f"{who}: contours must hold triangles, (S, 3, 3) (got points of shape {c.points.shape}: "
                             "level curves of a 2-D mesh are not surfaces)")
    pts = np.concatenate([c.points for c in cs]) if cs else np.zeros((0, 3, 3))
    T = int(pts.shape[0])
    if values is not None:
        V = np.asarray(values, dtype=np.float64)
        if V.shape == (T,):
            V = np.repeat(V[:, None], 3, axis=1)
        if V.shape != (T, 3):
            raise ValueError(f"{who}: values must be ({T},) or ({T}, 3) for these contours (got shape {V.shape})")
        return pts, V
    if levels is not None:
        levels = [levels] if single else list(levels)
        if len(levels) != len(cs):
            raise ValueError(f"{who}: levels must give one array of level values per contour ({len(cs)})")
    vals = []
    for i, c in enumerate(cs):
        if isinstance(c, Tessellation):
            if c.values is None:
                raise ValueError(f"{who}: a Tessellation without values needs values= (tessellate(geom, fields) gives "
                                 "it the fields at its vertices)")
            vals.append(c.values[..., 0])
        elif c.carried is not None:
            vals.append(c.carried[..., 0])
        elif levels is not None:
            lev = np.asarray(levels[i], dtype=np.float64).reshape(-1)
            if lev.shape[0] != c.nlevels:
                raise ValueError(f"{who}: levels[{i}] has {lev.shape[0]} values for a contour of {c.nlevels} levels")
            vals.append(np.repeat(lev[c.level][:, None], 3, axis=1))
        else:
            raise ValueError(f"{who}: a contour without carried fields needs values= or levels= (a Contour keeps the "
                             "index of each triangle's level, not its value)")
    return pts, (np.concatenate(vals) if vals else np.zeros((0, 3)))


def render_surfaces(contours, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0,
                    height: Optional[float] = None, values=None, levels=None, transfer=None, clim=None,
                    ambient: float = 0.3, max_hits: int = 1, device_id: int = 0):
    """`(image, depth)`: the `(H, W, 4)` premultiplied colour and alpha of the triangles of one `Contour` (3-D), one
    `Tessellation` of a surface in R^3 (`e = 3`) or a list mixing them, seen by the camera of `camera_rays`, row 0 at the
    top, and the `(H, W)` ray parameter of each pixel's first hit (`inf` where there is none).

    `values` is `(T,)` or `(T, 3)` over the concatenated triangles.  Its default is `values[..., 0]` for a tessellation
    (one with `e = 2`, or without values and without `values=`, raises `ValueError`), `carried[..., 0]` for a contour
    that carries fields and the level value per triangle otherwise, looked up in `levels` (the values given to
    `isocontour`; one array per contour, tessellations included: their entry is not read).  `transfer`, `clim` and
    `ambient` are those of `TriangleCaster.shade`.  The `max_hits` layers of a pixel are composited front to back
    (`composite_layers`).
    """
    who = "render_surfaces"
    pts, V = _soup(who, contours, values, levels)
    W, H = _check_size(size)
    o, d = camera_rays(eye, target, up, (W, H), fov, height)
    K = _check_max_hits(who, max_hits)
    T = default_surface_table() if transfer is None else _check_table(who, transfer)
    ambient = _check_ambient(who, ambient)
    if pts.shape[0] == 0:
        return np.zeros((H, W, 4)), np.full((H, W), np.inf)
    if not np.all(np.isfinite(pts)):
        raise ValueError(f"{who}: the contours have non-finite points")
    clim = _clim(who, clim, V, "values")
    with TriangleCaster(pts, device_id=device_id) as tc:
        hits = tc.trace(o, d, max_hits=K)
        layers = tc.shade(hits, d, V, T, clim, ambient)
    return composite_layers(layers).reshape(H, W, 4), hits.t[:, 0].reshape(H, W)


def _figure_lines(who: str, lines, line_radius, line_color) -> np.ndarray:
    """The segments `(S, 2, 3)` of `render_figure`'s `lines`, with `line_radius` and `line_color` checked."""
    from .tubes import _check_line_color, _check_radius, segments
    pts, _ = segments(lines, who=who)
    if not np.all(np.isfinite(pts)):
        raise ValueError(f"{who}: lines have non-finite points")
    if line_radius is not None:
        _check_radius(who, line_radius, int(pts.shape[0]), "line_radius")
    _check_line_color(who, line_color)
    return pts


def _merge_lines(who: str, seg_pts, o, d, line_radius, line_color, diagonal, ambient, device_id, t_hit, layers):
    """The triangles' `(t_hit, layers)` with the opaque layer of the segments merged in by depth."""
    from .tubes import _check_line_color, figure_line_layers, merge_layers
    lt, ll = figure_line_layers(who, seg_pts, o, d, line_radius, _check_line_color(who, line_color), diagonal, ambient,
                                device_id)
    return merge_layers((t_hit, layers), (lt, ll), max_hits=MAX_HITS)


def _render_surface_figure(geom: Geometry, u, eye, target, up, size, fov, isosurfaces, slices, volume, surface_alpha, step,
                           transfer, clim, ambient, refine, device_id, lines=None, line_radius=None,
                           line_color=(0.0, 0.0, 0.0)) -> np.ndarray:
    """`render_figure` on a `fem2d` surface in R^3: its tessellation traced and shaded once (plot3d.jl:239-256)."""
    who = "render_figure"
    for name, given in (("isosurfaces", isosurfaces is not None), ("slices", slices is not None),
                        ("volume=True", volume is True), ("step", step is not None)):
        if given:
            raise ValueError(f"{who}: {name} has no meaning for a fem2d surface in R^3 (the figure is the surface itself, "
                             "coloured by u)")
    from .contour import _check_tessellate
    W, H = _check_size(size)
    o, d = camera_rays(eye, target, up, (W, H), fov)
    p, N, _ = geom.x.shape
    U = np.asarray(u, dtype=np.float64)
    if U.ndim != 1 or U.shape[0] != p * N:
        raise ValueError(f"{who}: u must be a vector of {p * N} values for this fem2d geometry (got shape {U.shape})")
    try:
        _check_tessellate(geom, U, refine)
    except ValueError as e:
        raise ValueError(str(e).replace("tessellate:", f"{who}:", 1)) from None
    clim = _clim(who, clim, U, "u")
    table = default_transfer(1.0) if transfer is None else _check_transfer(transfer)      # its sigma column is replaced
    if not (isinstance(surface_alpha, (int, float, np.integer, np.floating)) and 0.0 <= surface_alpha <= 1.0):
        raise ValueError(f"{who}: surface_alpha must be a number in [0, 1] (got {surface_alpha!r})")
    ambient = _check_ambient(who, ambient)
    levels = seg_pts = None
    if lines is not None:
        if isinstance(lines, (list, tuple, np.ndarray)) and all(isinstance(v, (int, float, np.integer, np.floating))
                                                                 and not isinstance(v, bool) for v in lines):
            levels = np.asarray(lines, dtype=np.float64).reshape(-1)           # level values: cut below, on the device
            if not np.all(np.isfinite(levels)):
                raise ValueError(f"{who}: every level value of lines must be finite")
            _figure_lines(who, np.zeros((0, 2, 3)), None, line_color)
            if line_radius is not None and not (isinstance(line_radius, (int, float, np.integer, np.floating))
                                                and math.isfinite(line_radius) and line_radius > 0.0):
                raise ValueError(f"{who}: line_radius must be a positive finite number when lines holds level values "
                                 f"(got {line_radius!r})")
        else:
            seg_pts = _figure_lines(who, lines, line_radius, line_color)
    tess = tessellate(geom, U, refine, device_id=device_id)
    surf_table = table.copy()
    surf_table[:, 3] = float(surface_alpha)
    K = 1 if surface_alpha == 1 else 4
    with TriangleCaster(tess.points, device_id=device_id) as tc:
        hits = tc.trace(o, d, max_hits=K)
        layers = tc.shade(hits, d, tess.values[..., 0], surf_table, clim, ambient)
    if levels is not None and levels.size:
        seg_pts = isocontour(geom, U, levels, refine, device_id=device_id).points
    if seg_pts is not None and seg_pts.shape[0]:
        nodes = geom.xflat
        diagonal = _diagonal(np.stack([nodes.min(axis=0), nodes.max(axis=0)]))
        _, layers = _merge_lines(who, seg_pts, o, d, line_radius, line_color, diagonal, ambient, device_id, hits.t, layers)
    return composite_layers(layers).reshape(H, W, 4)


def render_figure(geom: Geometry, u, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0, isosurfaces=None,
                  slices=None, volume: Optional[bool] = None, surface_alpha: float = 1.0, step: Optional[float] = None,
                  transfer=None, clim=None, ambient: float = 0.3, device_id: int = 0,
                  refine: Optional[int] = None, lines=None, line_radius=None,
                  line_color=(0.0, 0.0, 0.0)) -> np.ndarray:
    """`(H, W, 4)`: the reference's default figure of the `fem3d` solution `u`: the volume render of `render_volume` with
    isosurfaces and slices composited into it at their depth, row 0 at the top.

    For a `fem2d` surface in R^3 (`fem2d(K=..., ambient=3)`) the figure is the reference's picture of a solution on a
    surface (plot3d.jl:182-256): `tessellate(geom, u, refine)` traced and shaded once by `TriangleCaster`, coloured by
    `u` through `transfer` / `clim` with the alpha `surface_alpha`.  `refine` is that of `tessellate`; `isosurfaces`,
    `slices`, `volume=True` and `step` given explicitly raise `ValueError` there: they have no meaning on a surface.
    Everything below is about `fem3d`, where `refine` must stay None.

    - `isosurfaces`: the level values; the default is the reference's `[0.1, 0.3, 0.5, 0.7, 0.9] * (max - min) + min`
      over the finite entries of `u`; `[]` draws none.  Their triangles are coloured by their level value.
    - `slices`: a list of `(axis, coordinate)` pairs, each the plane `x[axis] = coordinate` cut by
      `isocontour(geom, geom.xflat[:, axis], [coordinate], carry=u)` and coloured by `u` on it.
    - `volume=False` gives the surfaces alone; the default (None) is True for `fem3d`.
    - `transfer` (`(K, 4)`: `r, g, b, sigma`; the default is that of `render_volume`) and `clim` are shared: the surfaces
      take the table's colours with the alpha `surface_alpha` in place of `sigma`.  A pixel keeps its nearest hit when
      `surface_alpha == 1` and its four nearest otherwise.
    - `step` is the sample distance of the volume (the default is 1/256 of the clip box's diagonal).
    - `lines` (anything `tubes.segments()` takes: `Streamlines`, level curves in R^3, `(S, 2, 3)` arrays, a list of them)
      are drawn into the figure as opaque tubes of the colour `line_color` and the radius `line_radius` (a number or
      one per segment; the default is 0.01 x the clip box's diagonal): a `SegmentCaster` traces them, `merge_layers`
      merges their layer with the triangles' by depth.  On a surface `lines` may also be a 1-D array of level values
      and then means `isocontour(geom, u, lines)`, drawn on the surface; the default radius there is 0.01 x the
      diagonal of the nodes' box.  With `lines=None` nothing of this runs.
    """
    who = "render_figure"
    disc = geom.discretization
    if isinstance(disc, TensorFEM) and disc.d == 2 and disc.e == 3:
        return _render_surface_figure(geom, u, eye, target, up, size, fov, isosurfaces, slices, volume, surface_alpha, step,
                                      transfer, clim, ambient, refine, device_id, lines, line_radius, line_color)
    _, name, dim, _, p, N, _, _ = _raycast_plan(geom, who)
    if refine is not None:
        raise ValueError(f"{who}: refine is for a fem2d surface in R^3 (tessellate); {name} geometries do not take it")
    volume = True if volume is None else volume
    if dim != 3:
        raise ValueError(f"{who}: {name} geometries are not supported (the camera is 3-D: fem3d only)")
    W, H = _check_size(size)
    o, d = camera_rays(eye, target, up, (W, H), fov)
    U = np.asarray(u, dtype=np.float64)
    if U.ndim != 1 or U.shape[0] != p * N:
        raise ValueError(f"{who}: u must be a vector of {p * N} values for this {name} geometry (got shape {U.shape})")
    clim = _clim(who, clim, U, "u")
    box = clip_box(geom)
    table = default_transfer(_diagonal(box)) if transfer is None else _check_transfer(transfer)
    if not (isinstance(surface_alpha, (int, float, np.integer, np.floating)) and 0.0 <= surface_alpha <= 1.0):
        raise ValueError(f"{who}: surface_alpha must be a number in [0, 1] (got {surface_alpha!r})")
    ambient = _check_ambient(who, ambient)
    if isosurfaces is None:
        fin = U[np.isfinite(U)]
        lev = np.array(REFERENCE_ISOSURFACES) * (float(fin.max()) - float(fin.min())) + float(fin.min())
    else:
        lev = np.asarray(isosurfaces, dtype=np.float64).reshape(-1)
        if not np.all(np.isfinite(lev)):
            raise ValueError(f"{who}: every entry of isosurfaces must be finite")
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
    if step is None:
        step = _diagonal(box) / 256.0
    elif not (isinstance(step, (int, float, np.integer, np.floating)) and math.isfinite(step) and step > 0.0):
        raise ValueError(f"{who}: step must be finite and positive (got {step!r})")
    seg_pts = None if lines is None else _figure_lines(who, lines, line_radius, line_color)
    # the soup: isosurfaces coloured by their level value, slices by the carried u
    pts, vals = [], []
    if lev.size:
        iso = isocontour(geom, U, lev, device_id=device_id)
        pts.append(iso.points)
        vals.append(np.repeat(lev[iso.level][:, None], 3, axis=1))
    for axis, coord in planes:
        cut = isocontour(geom, geom.xflat[:, axis], [coord], carry=U, device_id=device_id)
        pts.append(cut.points)
        vals.append(cut.carried[..., 0])
    pts = np.concatenate(pts) if pts else np.zeros((0, 3, 3))
    vals = np.concatenate(vals) if vals else np.zeros((0, 3))
    surf_table = table.copy()
    surf_table[:, 3] = float(surface_alpha)
    K = 1 if surface_alpha == 1 else 4
    with TriangleCaster(pts, device_id=device_id) as tc:
        hits = tc.trace(o, d, max_hits=K)
        layers = tc.shade(hits, d, vals, surf_table, clim, ambient)
    t_hit = hits.t
    if seg_pts is not None and seg_pts.shape[0]:
        t_hit, layers = _merge_lines(who, seg_pts, o, d, line_radius, line_color, _diagonal(box), ambient, device_id,
                                     t_hit, layers)
    if not volume:
        return composite_layers(layers).reshape(H, W, 4)
    with RayCaster(geom, o, d, step, device_id=device_id) as rc:
        return rc.render(U, table, clim, layers=(t_hit, layers)).reshape(H, W, 4)
