"""Level curves as ordered lines: `polylines(curves)` orders the segments of a curve mesh into open and closed polylines.

The reference gets ordered, indexed PolyData from PyVista.  Here `isocontour()`, the boundary edges of a welded surface and
a welded `Streamlines` are unordered segments in launch order and random orientation; `weld()` indexes them and
`polylines()` orders them on the device in one call of `mgbhip_polyline_create` (csrc/polyline.hip: list ranking by
pointer doubling).  The host only checks arguments, gathers the per-point data and offers the small queries that belong
with the type (`lines()`, `reversed()`, `at()`, `resample()`, `save()`); `at()` samples on the device through
`mgbhip_polyline_sample`.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .contour import Contour, Tessellation
from .streamlines import Streamlines
from .weld import IndexedMesh, weld


@dataclass
class Polylines:
    """What `polylines()` returns: `L` lines over `P` points.  Line `l` of `n` edges owns the `n + 1` points
    `offsets[l] : offsets[l + 1]`; a closed line repeats its first vertex as its last point."""
    offsets: np.ndarray                  # (L + 1,) int64
    vertex: np.ndarray                   # (P,) int32: the mesh vertex of every point
    segment: np.ndarray                  # (P,) int32: the segment from point j to j + 1; -1 at the last point of a line
    closed: np.ndarray                   # (L,) uint8
    arclength: np.ndarray                # (P,) float64: 0 at the first point of a line, then the running length
    length: np.ndarray                   # (L,) float64: the arc length at the last point of every line
    points: np.ndarray                   # (P, e) float64: vertices[vertex]
    vertex_data: Optional[np.ndarray]    # (P, C) float64: the mesh's vertex_data[vertex], or None
    level: Optional[np.ndarray]          # (L,) int32: the mesh's level of every line's first segment, or None
    ndropped: int                        # segments with two equal vertices, or repeating a lower-numbered segment
    rounds: Tuple[int, ...]              # pointer-doubling rounds of the cycle pass and of the ranking pass
    cells: np.ndarray                    # (S, 2) int32: the segments that were ordered
    mesh: Optional[IndexedMesh] = None   # the welded mesh, when the input was a mesh or was welded first
    device_id: int = 0

    @property
    def nlines(self) -> int:
        return int(self.offsets.shape[0]) - 1

    def lines(self):
        """A list of `(n_l + 1, e)` views of `points`, one per line."""
        o = self.offsets
        return [self.points[o[l]:o[l + 1]] for l in range(self.nlines)]

    def reversed(self) -> np.ndarray:
        """(P,) bool: true where segment `segment[j]` is traversed from its second corner to its first (false at the last
        point of a line)."""
        out = np.zeros(self.vertex.shape[0], dtype=bool)
        has = self.segment >= 0
        out[has] = self.cells[self.segment[has], 1] == self.vertex[has]
        return out

    def at(self, line, s):
        """The points at arc length `s` of line `line` (both broadcast to `(Q,)`): `s` is clamped to `[0, length[line]]`,
        `j` is the last edge of the line whose first point has `arclength <= s`, and the point is
        `x_j + t (x_{j+1} - x_j)` with `t = (s - a_j) / (a_{j+1} - a_j)` (0 on an edge of length 0).  Returns `(Q, e)`
        points, and `(points, data (Q, C))` when the lines have `vertex_data`.  Evaluated on the device."""
        ln, sv = _check_queries(self, line, s)
        Q, e = ln.shape[0], self.points.shape[1]
        D = self.vertex_data
        Cn = 0 if D is None else int(D.shape[1])
        out = np.empty((Q, e))
        od = None if D is None else np.empty((Q, Cn))
        if Q:
            from .device import ERR_INVALID, HipContext, MGBHipError, _check as _status, _ptr
            ctx = HipContext(self.device_id)
            try:
                pts = np.ascontiguousarray(self.points, dtype=np.float64)
                dat = None if D is None else np.ascontiguousarray(D, dtype=np.float64)
                off = np.ascontiguousarray(self.offsets, dtype=np.int64)
                arc = np.ascontiguousarray(self.arclength, dtype=np.float64)
                try:
                    _status(ctx.lib, ctx.lib.mgbhip_polyline_sample(
                        ctx.handle, e, pts.shape[0], _ptr(pts), Cn, _ptr(dat), self.nlines,
                        off.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(arc), Q, ln.ctypes.data_as(C.POINTER(C.c_int32)),
                        _ptr(sv), _ptr(out), _ptr(od)))
                except MGBHipError as err:
                    if err.status == ERR_INVALID:
                        raise ValueError(str(err)) from None
                    raise
            finally:
                ctx.close()
        return out if D is None else (out, od)

    def abscissae(self, n=None, spacing=None):
        """`(line (Q,) int32, s (Q,) float64, offsets (L + 1,) int64)`: the arc lengths `resample()` evaluates.  Exactly
        one of `n` (points per line) and `spacing` is given.  An open line gets `i * (length / (n - 1))` with the last
        set to `length` (`n >= 2`), a closed line `i * (length / n)`, `i < n` (`n >= 3`); with `spacing = h`,
        `n = max(2, ceil(length / h) + 1)` for an open line and `max(3, ceil(length / h))` for a closed one."""
        if (n is None) == (spacing is None):
            raise ValueError("resample: give exactly one of n and spacing")
        L = self.nlines
        if n is not None:
            if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
                raise ValueError(f"resample: n must be an integer (got {n!r})")
            if n < 2 or (n < 3 and np.any(self.closed)):
                raise ValueError(f"resample: n must be >= 2, and >= 3 when a line is closed (got {n})")
            counts = np.full(L, int(n), dtype=np.int64)
        else:
            if isinstance(spacing, bool) or not isinstance(spacing, (int, float, np.integer, np.floating)):
                raise ValueError(f"resample: spacing must be a number (got {spacing!r})")
            h = float(spacing)
            if not (np.isfinite(h) and h > 0.0):
                raise ValueError(f"resample: spacing must be finite and > 0 (got {spacing!r})")
            counts = np.array([max(3, math.ceil(self.length[l] / h)) if self.closed[l]
                               else max(2, math.ceil(self.length[l] / h) + 1) for l in range(L)], dtype=np.int64)
        offsets = np.zeros(L + 1, dtype=np.int64)
        np.cumsum(counts, out=offsets[1:])
        line = np.repeat(np.arange(L, dtype=np.int32), counts)
        s = np.empty(int(offsets[-1]))
        for l in range(L):
            k, ln = int(counts[l]), float(self.length[l])
            i = np.arange(k, dtype=np.float64)
            if self.closed[l]:
                s[offsets[l]:offsets[l + 1]] = i * (ln / k)
            else:
                s[offsets[l]:offsets[l + 1]] = i * (ln / (k - 1))
                s[offsets[l + 1] - 1] = ln
        return line, s, offsets

    def resample(self, n=None, spacing=None):
        """Every line resampled at the arc lengths of `abscissae(n, spacing)`: `(points, offsets)`, or
        `(points, offsets, data)` when the lines have `vertex_data`."""
        line, s, offsets = self.abscissae(n, spacing)
        got = self.at(line, s)
        if self.vertex_data is None:
            return got, offsets
        return got[0], offsets, got[1]

    def save(self, path) -> None:
        """Write the lines as ASCII Wavefront `.obj` (one `v` per point, one `l` record per line) or legacy ASCII `.vtk`
        POLYDATA (one `LINES` cell per line; `arclength` and `vertex_data` as POINT_DATA, `closed` and `level` as
        CELL_DATA), chosen by the suffix of `path`; coordinates with 17 significant digits.  The points are the `P`
        points of the lines, so a closed line ends on a copy of its first point.  2-D lines are written with a third
        coordinate of 0.  Any other suffix raises `ValueError`."""
        suffix = os.path.splitext(str(path))[1].lower()
        if suffix not in (".obj", ".vtk"):
            raise ValueError(f"Polylines.save: the suffix must be .obj or .vtk (got {str(path)!r})")
        X = self.points
        if X.shape[1] == 2:
            X = np.concatenate([X, np.zeros((X.shape[0], 1))], axis=1)
        P, L, o = X.shape[0], self.nlines, self.offsets
        num = lambda row: " ".join("%.17g" % v for v in row)     # noqa: E731
        out = []
        if suffix == ".obj":
            out.append("# multigridbarrier polylines: %d points, %d lines" % (P, L))
            out += ["v " + num(p) for p in X]
            out += ["l " + " ".join("%d" % (j + 1) for j in range(o[l], o[l + 1])) for l in range(L)]
        else:
            out += ["# vtk DataFile Version 3.0", "multigridbarrier polylines", "ASCII", "DATASET POLYDATA",
                    "POINTS %d double" % P]
            out += [num(p) for p in X]
            out.append("LINES %d %d" % (L, L + P))
            out += [("%d " % (o[l + 1] - o[l])) + " ".join("%d" % j for j in range(o[l], o[l + 1])) for l in range(L)]
            out += ["CELL_DATA %d" % L, "SCALARS closed int 1", "LOOKUP_TABLE default"]
            out += ["%d" % v for v in self.closed]
            if self.level is not None:
                out += ["SCALARS level int 1", "LOOKUP_TABLE default"]
                out += ["%d" % v for v in self.level]
            out += ["POINT_DATA %d" % P, "SCALARS arclength double 1", "LOOKUP_TABLE default"]
            out += ["%.17g" % v for v in self.arclength]
            if self.vertex_data is not None:
                for j in range(self.vertex_data.shape[1]):
                    out += ["SCALARS data%d double 1" % j, "LOOKUP_TABLE default"]
                    out += ["%.17g" % v for v in self.vertex_data[:, j]]
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")


def _check_queries(pl: Polylines, line, s):
    """The argument checks of `Polylines.at()`; `(line (Q,) int32, s (Q,) float64)`."""
    try:
        ln = np.asarray(line)
        sv = np.asarray(s, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("Polylines.at: line must be integers and s numbers") from None
    if not np.issubdtype(ln.dtype, np.integer):
        raise ValueError(f"Polylines.at: line must be integers (got dtype {ln.dtype})")
    try:
        ln, sv = np.broadcast_arrays(ln, sv)
    except ValueError:
        raise ValueError(f"Polylines.at: line and s do not broadcast (shapes {ln.shape} and {sv.shape})") from None
    ln, sv = ln.reshape(-1), sv.reshape(-1)
    if ln.size and (ln.min() < 0 or ln.max() >= pl.nlines):
        raise ValueError(f"Polylines.at: line must lie in [0, {pl.nlines}) (got {int(ln.min())} .. {int(ln.max())})")
    if not np.all(np.isfinite(sv)):
        raise ValueError("Polylines.at: s must be finite")
    return np.ascontiguousarray(ln, dtype=np.int32), np.ascontiguousarray(sv, dtype=np.float64)


def _check(curves, tol):
    """Every argument check of `polylines()` that needs no welding: `(vertices, cells, mesh or None, soup or None)`."""
    mesh = soup = None
    if isinstance(curves, IndexedMesh):
        if curves.cells.ndim != 2 or curves.cells.shape[1] != 2:
            raise ValueError("polylines: an IndexedMesh must hold segments, nv = 2 (got cells of shape "
                             f"{curves.cells.shape}; for the boundary loops of a surface pass (w.vertices, "
                             "w.boundary_edges()))")
        mesh, Vx, cells = curves, curves.vertices, curves.cells
    elif isinstance(curves, (Contour, Streamlines)):
        if isinstance(curves, Contour):
            shp = np.asarray(curves.points).shape
            if len(shp) != 3 or shp[1] != 2:
                raise ValueError(f"polylines: a Contour must hold segments, (S, 2, e) (got points of shape {shp})")
        return None, None, None, curves
    elif isinstance(curves, Tessellation):
        raise ValueError("polylines: a Tessellation holds triangles, not curves")
    elif isinstance(curves, (tuple, list)) and len(curves) == 2:
        Vx, cells = curves
    else:
        raise ValueError("polylines: curves must be an IndexedMesh of segments, a Contour of segments, a Streamlines or a "
                         f"pair (vertices (V, e), cells (S, 2)) (got {type(curves).__name__})")
    if tol is not None:
        raise ValueError("polylines: tol applies only to a Contour or a Streamlines, which are welded first")
    try:
        Vx = np.asarray(Vx, dtype=np.float64)
        cells = np.asarray(cells)
    except (TypeError, ValueError):
        raise ValueError("polylines: vertices must be a (V, e) float array and cells an (S, 2) integer array") from None
    if Vx.ndim != 2 or Vx.shape[1] not in (2, 3):
        raise ValueError(f"polylines: vertices must be (V, e) with e in {{2, 3}} (got shape {Vx.shape})")
    if cells.ndim != 2 or cells.shape[1] != 2 or not (np.issubdtype(cells.dtype, np.integer) or cells.size == 0):
        raise ValueError(f"polylines: cells must be (S, 2) integers (got shape {cells.shape}, dtype {cells.dtype})")
    if 2 * cells.shape[0] >= 2 ** 31:
        raise ValueError("polylines: S x 2 half-edges exceed 32-bit indexing (2 S >= 2^31)")
    if cells.size and (cells.min() < 0 or cells.max() >= Vx.shape[0]):
        raise ValueError(f"polylines: the entries of cells must lie in [0, V = {Vx.shape[0]}) (got {int(cells.min())} .. "
                         f"{int(cells.max())})")
    if not np.all(np.isfinite(Vx)):
        raise ValueError("polylines: vertices has a non-finite coordinate")
    return np.ascontiguousarray(Vx), np.ascontiguousarray(cells, dtype=np.int32), mesh, None


def polylines(curves, tol: Optional[float] = None, device_id: int = 0) -> Polylines:
    """Order the segments of a curve mesh into polylines.

    `curves` is an `IndexedMesh` of segments (`nv = 2`), a `Contour` of segments or a `Streamlines` (welded first with
    `weld(curves, tol)`; the mesh is kept as `.mesh`), or a pair `(vertices (V, e), cells (S, 2))`, for example
    `(w.vertices, w.boundary_edges())` for the boundary loops of a welded surface.

    - A segment is dropped if its two vertices are equal, or if a lower-numbered segment that is not dropped joins the
      same two vertices; the others are edges, and `ndropped` counts the dropped.
    - A vertex with two edges is interior; one with one edge (an end) or three and more (a junction) is a node.  Edges that
      share an interior vertex belong to one line, so a line is an open path between two nodes (which may be the same
      junction) or a cycle of interior vertices (closed).
    - Lines are numbered by their lowest segment.  An open line starts at the end with the smaller vertex number (with
      equal ends, along the end edge with the lower segment number); a closed line starts at its lowest vertex and goes on
      to the smaller of that vertex's two neighbours.
    - `arclength` is the running sum of `sqrt((dx*dx + dy*dy) [+ dz*dz])` within each line.

    Every refusal is a `ValueError` raised before any device work.  An empty input returns an empty `Polylines` without
    touching the device.  Two calls return bitwise equal arrays.
    """
    Vx, cells, mesh, soup = _check(curves, tol)
    if soup is not None:
        mesh = weld(soup, tol, device_id=device_id)
        Vx, cells = np.ascontiguousarray(mesh.vertices, dtype=np.float64), np.ascontiguousarray(mesh.cells, dtype=np.int32)
    V, e = (int(v) for v in Vx.shape)
    S = int(cells.shape[0])
    vdata = None if mesh is None else mesh.vertex_data
    mlevel = None if mesh is None else mesh.level
    if S == 0:
        return Polylines(np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32),
                         np.zeros(0, dtype=np.uint8), np.zeros(0), np.zeros(0), np.zeros((0, e)),
                         None if vdata is None else np.zeros((0, vdata.shape[1])),
                         None if mlevel is None else np.zeros(0, dtype=np.int32), 0, (0, 0), cells, mesh, device_id)
    from .device import ERR_INVALID, HipContext, MGBHipError, _check as _status, _ptr
    ip, lp = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    ctx = HipContext(device_id)
    handle = None
    try:
        h = C.c_void_p()
        nL, nP, nD = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        try:
            _status(ctx.lib, ctx.lib.mgbhip_polyline_create(ctx.handle, V, e, _ptr(Vx), S, cells.ctypes.data_as(ip), C.byref(h),
                                                            C.byref(nL), C.byref(nP), C.byref(nD)))
        except MGBHipError as err:
            if err.status == ERR_INVALID:
                raise ValueError(str(err)) from None
            raise
        handle = h
        L, P = int(nL.value), int(nP.value)
        offsets = np.empty(L + 1, dtype=np.int64)
        vertex, segment = np.empty(P, dtype=np.int32), np.empty(P, dtype=np.int32)
        closed = np.empty(L, dtype=np.uint8)
        arclength, length = np.empty(P), np.empty(L)
        _status(ctx.lib, ctx.lib.mgbhip_polyline_fetch(handle, offsets.ctypes.data_as(lp), vertex.ctypes.data_as(ip),
                                                       segment.ctypes.data_as(ip), closed.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                       _ptr(arclength), _ptr(length)))
        rounds = (C.c_int32 * 8)()
        nph = C.c_int32(0)
        _status(ctx.lib, ctx.lib.mgbhip_polyline_rounds(handle, rounds, C.byref(nph)))
    finally:
        if handle is not None:
            ctx.lib.mgbhip_polyline_destroy(handle)
        ctx.close()
    first = segment[offsets[:-1]]
    return Polylines(offsets, vertex, segment, closed, arclength, length, Vx[vertex],
                     None if vdata is None else vdata[vertex], None if mlevel is None else np.asarray(mlevel)[first],
                     int(nD.value), tuple(int(rounds[i]) for i in range(nph.value)), cells, mesh, device_id)
