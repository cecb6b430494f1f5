"""Curves drawn as tubes: `SegmentCaster` (nearest hits of rays with a soup of capsules and their shading),
`segments()` / `curve_segments()` (the segments of field lines, level curves and `fem1d` curves), `merge_layers()`,
`render_lines(lines, eye, target)` and `render_curve(geom, z, eye, target)`.

The reference draws a `fem1d` curve in R^2 / R^3 as a tube coloured by the solution
(ext/MultiGridBarrierPyPlotExt/plot3d.jl:209-224 and :279-308; the default radius of `poly.tube` is 1 % of the
bounding-box diagonal).  `streamlines()` on a `fem3d` mesh and `isocontour()` on a `fem2d` surface in R^3 give curves in
R^3 as well.  Here every such curve is a soup of segments with a radius each -- capsules: a cylinder body with a
spherical cap at each end -- traced on the device (csrc/tubes.hip) like the triangles of `TriangleCaster`, and its
layers go into `RayCaster.render(..., layers=...)` next to the triangles' (`merge_layers`).  The host only checks
arguments (before any device work), normalises the directions and concatenates soups.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._handle import DeviceObject
from .contour import Contour
from .interpolate import _c_f64
from .multigrid import Geometry
from .polyline import Polylines
from .raycast import _check_size, camera_rays
from .streamlines import Streamlines
from .surface import (MAX_HITS, _check_ambient, _check_colouring, _check_hits, _check_max_hits, _check_rays, _check_table,
                      _clim, _trace_arguments, composite_layers, default_surface_table)
from .tensorfem import TensorFEM

REFERENCE_RADIUS = 0.01     # plot3d.jl:300-301: the tube radius as a fraction of the bounding-box diagonal


@dataclass
class TubeHits:
    """The `K` nearest hits of `R` rays, nearest first; a missing entry is `t = inf`, `segment = -1`, `s = NaN`."""
    t: np.ndarray            # (R, K) float64: the ray parameter (arc length) where the ray enters the capsule
    segment: np.ndarray      # (R, K) int32
    s: np.ndarray            # (R, K) float64: the nearest point of the axis is a + s (b - a); 0 / 1 on the caps


def _check_radius(who: str, radius, S: int, name: str = "radius") -> np.ndarray:
    try:
        r = np.asarray(radius, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} must be a positive finite number or ({S},) of them (got {radius!r})") from None
    if r.ndim == 0:
        r = np.full(S, float(r))
    if r.shape != (S,):
        raise ValueError(f"{who}: {name} must be a positive finite number or ({S},) of them (got shape {r.shape})")
    if not np.all(np.isfinite(r) & (r > 0.0)):
        raise ValueError(f"{who}: every {name} must be finite and positive")
    return r


class SegmentCaster(DeviceObject):
    """A soup of segments `points` (`(S, 2, 3)`: segment, end point, coordinate; finite) with a `radius` each (a positive
    finite number, or `(S,)` of them), sorted once into a uniform grid of cells on the device, for tracing many bundles
    of rays against the capsules around them.  `S = 0` is allowed: every ray misses and no device work is done.

    The capsule test (the same on the device and in the NumPy restatement the tests compare it with,
    tests/tubes_twin.py), for the ray `o + t dn` with `dn = d / sqrt(sum d*d)`, the end points `a`, `b` and the radius
    `r`, in IEEE double without fused multiply-adds, with `a . b = (a0*b0 + a1*b1) + a2*b2`:

        ba = b - a;  oa = o - a;  ob = o - b
        baba = ba.ba;  bard = ba.dn;  baoa = ba.oa;  rdoa = dn.oa;  oaoa = oa.oa
        A = baba - bard*bard;  B = baba*rdoa - baoa*bard;  Cq = (baba*oaoa - baoa*baoa) - (r*r)*baba;  h = B*B - A*Cq
        side:   valid iff A > 0, h >= 0 and 0 <= y <= baba with ts = (-B - sqrt(h))/A, y = baoa + ts*bard;  s = y/baba
        cap a:  b2 = dn.oa;  c2 = oaoa - r*r;  h2 = b2*b2 - c2;  valid iff h2 >= 0;  ta = -b2 - sqrt(h2);  s = 0
        cap b:  the same with ob;  s = 1

    The ray enters the capsule at the smallest valid one of `ts, ta, tb` (a tie keeps the earlier piece); the capsule is
    hit iff a piece is valid and `t_min <= t <= t_max` for that entry.  So a ray whose origin lies inside a capsule does
    not hit it, exit points are never reported, and a capsule gives at most one hit.  A ray keeps its `max_hits`
    nearest hits in the order of `(t, segment index)`.  Which capsules a ray is tested against is decided by the grid;
    what it hits is not.

    Use it as a context manager or call `close()`.
    """

    _closed_message = "SegmentCaster: the caster is closed"
    _destroy = "mgbhip_tubes_destroy"

    def __init__(self, points, radius, device_id: int = 0):
        P = np.asarray(points, dtype=np.float64)
        if P.ndim != 3 or P.shape[1:] != (2, 3):
            raise ValueError(f"SegmentCaster: points must be (S, 2, 3) (got shape {P.shape})")
        if not np.all(np.isfinite(P)):
            raise ValueError("SegmentCaster: every entry of points must be finite")
        self.nsegments = S = int(P.shape[0])
        rad = _check_radius("SegmentCaster", radius, S)
        if S:
            from .device import _ptr
            self._create(device_id, "mgbhip_tubes_create", S, _ptr(_c_f64(P)), _ptr(_c_f64(rad)))

    def trace(self, o, d, t_min: float = 0.0, t_max: float = np.inf, max_hits: int = 1) -> TubeHits:
        """The `max_hits` (1..8) nearest hits of every ray `o + t d` (`(R, 3)` each; one ray may be given as `(3,)`) with
        `t_min <= t <= t_max`; `t` is arc length."""
        self._open()
        O, Dn, t_min, t_max, K, t, seg, (s,) = _trace_arguments("SegmentCaster.trace", o, d, t_min, t_max, max_hits, 1)
        R = int(O.shape[0])
        if R and self.nsegments:
            from .device import _check, _ptr
            O, Dn = _c_f64(O), _c_f64(Dn)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_tubes_trace(
                self._handle, R, _ptr(O), _ptr(Dn), t_min, t_max, K, _ptr(t), seg.ctypes.data_as(C.POINTER(C.c_int32)),
                _ptr(s)))
        return TubeHits(t, seg, s)

    def shade(self, hits: TubeHits, o, d, values, transfer=None, clim=None, ambient: float = 0.3) -> np.ndarray:
        """`(R, K, 4)` float64: premultiplied colour and alpha of every hit.

        `o`, `d` are the rays the hits were traced with, `values` is `(S, 2)`: a value per segment end point.  The value
        of a hit is `c = (1 - s) c0 + s c1`; its row of `transfer` (`(K, 4)`: `r, g, b, alpha`; the default is
        `default_surface_table()`) is found as `TriangleCaster.shade` finds it, between `clim = (lo, hi)` (the default is
        the minimum and maximum of the finite `values`).  With `x = o + t dn`, `q = a + s (b - a)`, `n = x - q`,
        `nn = n / sqrt(n . n)` and `shade = ambient + (1 - ambient) |nn . dn|`, the layer is `alpha shade (r, g, b)` and
        `alpha = min(1, max(0, row[3]))`.  A missing hit or a non-finite `c` gives a zero layer.
        """
        self._open()
        who = "SegmentCaster.shade"
        if not isinstance(hits, TubeHits):
            raise ValueError(f"{who}: hits must be what trace() returned (got {type(hits).__name__})")
        O, Dn = _check_rays(who, o, d)
        R = int(Dn.shape[0])
        seg, (ht, hs) = _check_hits(who, R, self.nsegments, "rays o, d", "segment", hits.segment, t=hits.t, s=hits.s)
        K = int(seg.shape[1])
        there = seg >= 0
        if not (np.all(np.isfinite(ht[there])) and np.all((hs[there] >= 0.0) & (hs[there] <= 1.0))):
            raise ValueError(f"{who}: every hit of hits needs a finite hits.t and a hits.s in [0, 1]")
        V, T, lo, hi, ambient = _check_colouring(who, values, (self.nsegments, 2), transfer, clim, ambient)
        layer = np.zeros((R, K, 4))
        if R and self.nsegments:
            from .device import _check, _ptr
            O, Dn, V, T, ht, hs = _c_f64(O), _c_f64(Dn), _c_f64(V), _c_f64(T), _c_f64(ht), _c_f64(hs)
            seg = np.ascontiguousarray(seg, dtype=np.int32)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_tubes_shade(
                self._handle, R, K, _ptr(O), _ptr(Dn), _ptr(ht), seg.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(hs),
                _ptr(V), int(T.shape[0]), _ptr(T), lo, hi, ambient, _ptr(layer)))
        return layer


# ---------------------------------------------------------------------------------------------------------------------
# where segments come from
# ---------------------------------------------------------------------------------------------------------------------

_FLAT = "the lines of a flat 2-D mesh are not in R^3"


def _segments_of(who: str, item, values):
    """`(points (S, 2, 3), values (S, 2) or None)` of one `Streamlines`, `Polylines`, `Contour` or array."""
    if isinstance(item, Polylines):
        P = np.asarray(item.points, dtype=np.float64)
        if P.ndim != 2 or P.shape[1] != 3:
            raise ValueError(f"{who}: {_FLAT} (got Polylines with points of shape {P.shape})")
        if values is None and item.vertex_data is not None:
            values = item.vertex_data[:, 0]
        j = np.nonzero(item.segment >= 0)[0]                      # point j and j + 1 are neighbours on one line
        V = None
        if values is not None:
            V = np.asarray(values, dtype=np.float64)
            if V.shape != (P.shape[0],):
                raise ValueError(f"{who}: values of a Polylines must be ({P.shape[0]},), one per point (got shape {V.shape})")
            V = np.stack([V[j], V[j + 1]], axis=1)
        return np.stack([P[j], P[j + 1]], axis=1).reshape(-1, 2, 3), V
    if isinstance(item, Streamlines):
        P = np.asarray(item.points, dtype=np.float64)
        if P.ndim != 3 or P.shape[2] != 3:
            raise ValueError(f"{who}: {_FLAT} (got Streamlines with points of shape {P.shape}; d = 3 is needed)")
        n = np.asarray(item.n).astype(np.int64)
        V = None
        if values is not None:
            V = np.asarray(values, dtype=np.float64)
            if V.shape != P.shape[:2]:
                raise ValueError(f"{who}: values of a Streamlines must be {P.shape[:2]}, one per line point (got shape "
                                 f"{V.shape})")
        j = np.arange(max(P.shape[1] - 1, 0))
        keep = j[None, :] + 1 < n[:, None]                       # (S, M - 1): points j and j + 1 are both valid
        pts = np.stack([P[:, :-1][keep], P[:, 1:][keep]], axis=1) if P.shape[1] else np.zeros((0, 2, 3))
        if V is not None:
            V = np.stack([V[:, :-1][keep], V[:, 1:][keep]], axis=1)
        return pts.reshape(-1, 2, 3), V
    if isinstance(item, Contour):
        P = np.asarray(item.points, dtype=np.float64)
        if P.ndim == 3 and P.shape[1:] == (2, 2):
            raise ValueError(f"{who}: {_FLAT} (got a Contour with points of shape {P.shape})")
        if P.ndim != 3 or P.shape[1:] != (2, 3):
            raise ValueError(f"{who}: a Contour must hold level curves in R^3, (S, 2, 3) (got points of shape {P.shape})")
        if values is None and item.carried is not None:
            values = item.carried[..., 0]
    else:
        try:
            P = np.asarray(item, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: lines must be a Streamlines, a Contour, an (S, 2, 3) array or a list of them (got "
                             f"{type(item).__name__})") from None
        if P.ndim == 3 and P.shape[1:] == (2, 2):
            raise ValueError(f"{who}: {_FLAT} (got an array of shape {P.shape})")
        if P.ndim != 3 or P.shape[1:] != (2, 3):
            raise ValueError(f"{who}: lines must be a Streamlines, a Contour, an (S, 2, 3) array or a list of them (got an "
                             f"array of shape {P.shape})")
    S = int(P.shape[0])
    V = None
    if values is not None:
        V = np.asarray(values, dtype=np.float64)
        if V.shape == (S,):
            V = np.repeat(V[:, None], 2, axis=1)
        if V.shape != (S, 2):
            raise ValueError(f"{who}: values must be ({S},) or ({S}, 2) for these segments (got shape {V.shape})")
    return P, V


def segments(lines, values=None, who: str = "segments"):
    """`(points (S, 2, 3), values (S, 2) or None)`: the segments of

    - a `Streamlines` with `d = 3`: the consecutive valid points of every line; `values`, if given, has the shape of
      `points[..., 0]`, one value per line point;
    - a `Polylines` in R^3: the consecutive points of every line; `values` is `(P,)`, one per point, and defaults to
      `vertex_data[:, 0]` when the lines have it;
    - a `Contour` whose points are `(S, 2, 3)` (the level curves of a `fem2d` surface in R^3); `values` (`(S,)` or
      `(S, 2)`) defaults to `carried[..., 0]` when it carries fields;
    - an `(S, 2, 3)` array, with `values` `(S,)` or `(S, 2)`;
    - a list mixing these, concatenated; `values` is then None or a list with one entry (or None) per item, and either
      every item ends up with values or none does.

    Anything with two coordinates raises `ValueError`: the lines of a flat 2-D mesh are not in R^3.
    """
    if isinstance(lines, (list, tuple)):
        items = list(lines)
        if values is None:
            vals = [None] * len(items)
        elif isinstance(values, (list, tuple)) and len(values) == len(items):
            vals = list(values)
        else:
            raise ValueError(f"{who}: values for a list of lines must be a list with one entry per item ({len(items)})")
        parts = [_segments_of(who, it, v) for it, v in zip(items, vals)]
        have = [v is not None for _, v in parts]
        if any(have) and not all(have):
            raise ValueError(f"{who}: some items of lines have values and some have none; give values for all or for none")
        pts = np.concatenate([p for p, _ in parts]) if parts else np.zeros((0, 2, 3))
        V = np.concatenate([v for _, v in parts]) if parts and all(have) else None
        return pts, V
    return _segments_of(who, lines, values)


def _family_name(geom: Geometry) -> str:
    disc = geom.discretization
    if isinstance(disc, TensorFEM):
        return f"fem{disc.d}d"
    name = type(disc).__name__
    return {"FEM2D_P1": "fem2d_P1", "FEM2D_P2": "fem2d_P2", "SPECTRAL1D": "spectral1d", "SPECTRAL2D": "spectral2d"}.get(name, name)


def curve_segments(geom: Geometry, z, height_scale: float = 1.0, who: str = "curve_segments"):
    """`(points (k N, 2, 3), values (k N, 2))`: the segments of a `fem1d` curve embedded in R^3, or in R^2 with
    `height_scale * z` as the third coordinate (the reference's height graph, plot3d.jl:293), with `z` at their end
    points.  Nodes `j` and `j + 1` of every element are joined (`create_vtk_line_connectivity`), element by element.  A
    flat `fem1d` (`e = 1`) and every other family raise `ValueError`."""
    disc = geom.discretization
    if not (isinstance(disc, TensorFEM) and disc.d == 1):
        raise ValueError(f"{who}: {_family_name(geom)} geometries are not supported (a fem1d curve in R^2 or R^3 is)")
    if disc.e == 1:
        raise ValueError(f"{who}: a flat fem1d geometry (e = 1) is not a curve in R^2 or R^3; give fem1d(K=..., ambient=2 or 3)")
    p, N, e = geom.x.shape
    Z = np.asarray(z, dtype=np.float64)
    if Z.ndim != 1 or Z.shape[0] != p * N:
        raise ValueError(f"{who}: z must be a vector of {p * N} values for this fem1d geometry (got shape {Z.shape})")
    if not (isinstance(height_scale, (int, float, np.integer, np.floating)) and math.isfinite(height_scale)):
        raise ValueError(f"{who}: height_scale must be a finite number (got {height_scale!r})")
    X = np.asarray(geom.x, dtype=np.float64).transpose(1, 0, 2)            # (N, p, e): element, node, coordinate
    Zn = Z.reshape(N, p)
    if e == 2:
        X = np.concatenate([X, (float(height_scale) * Zn)[..., None]], axis=2)
    pts = np.stack([X[:, :-1], X[:, 1:]], axis=2).reshape(-1, 2, 3)
    vals = np.stack([Zn[:, :-1], Zn[:, 1:]], axis=2).reshape(-1, 2)
    return pts, vals


def merge_layers(*pairs, max_hits: Optional[int] = None):
    """`(t, layer)`: the pairs `(t (R, K_i), layer (R, K_i, 4))` concatenated along the hit axis and sorted by `t` per
    ray, stably, so that ties keep the order of the arguments; cut to `max_hits` entries (the default is
    `min(8, sum K_i)`).  Every `t` must ascend along its ray with `inf` for missing entries, as `trace` returns it; the
    result does too, which is what `RayCaster.render(layers=...)` demands.  At most 16 entries per ray, merged on the host
    like `composite_layers`."""
    who = "merge_layers"
    if not pairs:
        raise ValueError(f"{who}: at least one (t, layer) pair is needed")
    ts, ls = [], []
    for i, pr in enumerate(pairs):
        try:
            t, layer = pr
        except (TypeError, ValueError):
            raise ValueError(f"{who}: argument {i} must be a (t, layer) pair") from None
        t, layer = np.asarray(t, dtype=np.float64), np.asarray(layer, dtype=np.float64)
        if t.ndim != 2 or not 1 <= t.shape[1] <= MAX_HITS or layer.shape != t.shape + (4,):
            raise ValueError(f"{who}: argument {i} must be t (R, K) and layer (R, K, 4) with K in 1..{MAX_HITS} (got shapes "
                             f"{t.shape} and {layer.shape})")
        if ts and t.shape[0] != ts[0].shape[0]:
            raise ValueError(f"{who}: argument {i} holds {t.shape[0]} rays, argument 0 holds {ts[0].shape[0]}")
        if np.isnan(t).any():
            raise ValueError(f"{who}: the t of argument {i} has a NaN (a missing entry is inf)")
        ts.append(t)
        ls.append(layer)
    total = sum(t.shape[1] for t in ts)
    if total > 2 * MAX_HITS:
        raise ValueError(f"{who}: {total} entries per ray; at most {2 * MAX_HITS} can be merged")
    if max_hits is None:
        K = min(MAX_HITS, total)
    else:
        K = _check_max_hits(who, max_hits)
    t, layer = np.concatenate(ts, axis=1), np.concatenate(ls, axis=1)
    order = np.argsort(t, axis=1, kind="stable")[:, :K]
    return np.take_along_axis(t, order, axis=1), np.take_along_axis(layer, order[..., None], axis=1)


# ---------------------------------------------------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------------------------------------------------

def default_radius(points: np.ndarray) -> float:
    """0.01 x the diagonal of the bounding box of the segments' end points: the reference's default for `poly.tube`."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    ext = P.max(axis=0) - P.min(axis=0)
    return REFERENCE_RADIUS * float(math.sqrt(float(np.sum(ext * ext))))


def _check_line_radius(who: str, radius, name: str, pts: np.ndarray, diagonal: Optional[float] = None):
    """The radii `(S,)` of `pts`: `radius`, or the default over `diagonal` (or over the segments' own box)."""
    S = int(pts.shape[0])
    if radius is None:
        if S == 0:
            return np.zeros(0)
        rad = REFERENCE_RADIUS * diagonal if diagonal is not None else default_radius(pts)
        if not rad > 0.0:
            raise ValueError(f"{who}: the segments span no extent to take the default {name} from; give {name}=")
        return np.full(S, rad)
    return _check_radius(who, radius, S, name)


def _render_segments(who, pts, V, eye, target, up, size, fov, radius, transfer, clim, ambient, max_hits, device_id):
    W, H = _check_size(size)
    o, d = camera_rays(eye, target, up, (W, H), fov)
    K = _check_max_hits(who, max_hits)
    T = default_surface_table() if transfer is None else _check_table(who, transfer)
    ambient = _check_ambient(who, ambient)
    if not np.all(np.isfinite(pts)):
        raise ValueError(f"{who}: the lines have non-finite points")
    rad = _check_line_radius(who, radius, "radius", pts)
    if pts.shape[0] == 0:
        return np.zeros((H, W, 4)), np.full((H, W), np.inf)
    if V is None:                                # drawn in the table's first colour
        V, clim = np.zeros((pts.shape[0], 2)), (0.0, 1.0)
    else:
        clim = _clim(who, clim, V, "values")
    with SegmentCaster(pts, rad, device_id=device_id) as sc:
        hits = sc.trace(o, d, max_hits=K)
        layers = sc.shade(hits, o, d, V, T, clim, ambient)
    return composite_layers(layers).reshape(H, W, 4), hits.t[:, 0].reshape(H, W)


def render_lines(lines, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0, radius=None, values=None,
                 transfer=None, clim=None, ambient: float = 0.3, max_hits: int = 1, device_id: int = 0):
    """`(image, depth)`: the `(H, W, 4)` premultiplied colour and alpha of `lines` (anything `segments()` takes, with its
    `values`) drawn as tubes, seen by the camera of `camera_rays`, row 0 at the top, and the `(H, W)` ray parameter of
    each pixel's first hit (`inf` where there is none).  `render_surfaces` for segments.

    `radius` is a number or one per segment; the default is 0.01 x the diagonal of the segments' bounding box, the
    reference's.  `transfer`, `clim` and `ambient` are those of `SegmentCaster.shade`; segments without values are drawn
    in the table's first colour.  The `max_hits` layers of a pixel are composited front to back (`composite_layers`).
    """
    who = "render_lines"
    pts, V = segments(lines, values, who=who)
    return _render_segments(who, pts, V, eye, target, up, size, fov, radius, transfer, clim, ambient, max_hits, device_id)


def render_curve(geom: Geometry, z, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0, radius=None,
                 height_scale: float = 1.0, transfer=None, clim=None, ambient: float = 0.3, max_hits: int = 1,
                 device_id: int = 0):
    """`(image, depth)`: the reference's picture of the solution `z` on a `fem1d` curve (plot3d.jl:279-308) in one call: a
    tube around `curve_segments(geom, z, height_scale)` coloured by `z` -- in place for a curve in R^3, as the height
    graph `(x, y, height_scale * z)` for a curve in R^2 -- traced and shaded by `SegmentCaster` and composited by
    `composite_layers`.  The other arguments are those of `render_lines`."""
    who = "render_curve"
    pts, V = curve_segments(geom, z, height_scale, who=who)
    return _render_segments(who, pts, V, eye, target, up, size, fov, radius, transfer, clim, ambient, max_hits, device_id)


def _check_line_color(who: str, line_color) -> np.ndarray:
    try:
        c = np.asarray(line_color, dtype=np.float64)
    except (TypeError, ValueError):
        c = np.zeros(0)
    if c.shape != (3,) or not np.all(np.isfinite(c)):
        raise ValueError(f"{who}: line_color must be three finite numbers (r, g, b) (got {line_color!r})")
    return c


def figure_line_layers(who: str, pts, o, d, line_radius, line_color, diagonal: float, ambient: float, device_id: int):
    """`(t (R, 1), layer (R, 1, 4))` of the segments `pts` for `render_figure`: traced with `max_hits = 1` (they are
    opaque) and shaded in `line_color` through a two-row constant table.  `line_radius` defaults to 0.01 x `diagonal`."""
    rad = _check_line_radius(who, line_radius, "line_radius", pts, diagonal)
    table = np.tile(np.concatenate([line_color, [1.0]]), (2, 1))
    with SegmentCaster(pts, rad, device_id=device_id) as sc:
        hits = sc.trace(o, d, max_hits=1)
        layer = sc.shade(hits, o, d, np.zeros((pts.shape[0], 2)), table, (0.0, 1.0), ambient)
    return hits.t, layer
