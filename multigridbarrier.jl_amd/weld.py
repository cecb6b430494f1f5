"""An indexed mesh from a simplex soup: `weld(soup)` gives vertices, cells, connected components and vertex normals.

The reference hands its grids to PyVista, whose contour filter returns indexed PolyData.  Here `isocontour()`,
`tessellate()` and `streamlines()` return unindexed soups, and the copies of a vertex that two neighbouring elements
compute can differ by rounding, so the soup does not weld by bit equality.  `weld()` welds it by tolerance on the device in
one call of `mgbhip_weld_create` (csrc/weld.hip); the host only checks arguments, gathers the per-vertex data and offers
the small queries that belong with the type (`edges()`, `is_closed()`, `euler_characteristic()`, `save()`).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .contour import Contour, Tessellation
from .streamlines import Streamlines

MAX_CELL = 1024          # csrc/weld.hpp WELD_MAX_CELL
DEFAULT_TOL_REL = 2.0 ** -27


@dataclass
class IndexedMesh:
    """What `weld()` returns: `V` vertices, the `S` simplices of the soup as rows of vertex numbers (aligned with the
    soup: simplex `s` of the soup is `cells[s]`), and what was asked for along with them."""
    vertices: np.ndarray                 # (V, e) float64: the soup's own coordinates of every vertex's first corner
    cells: np.ndarray                    # (S, nv) int32
    first_corner: np.ndarray             # (V,) int32: the lowest corner (simplex * nv + corner) of every vertex
    component: np.ndarray                # (V,) int32: the connected component of every vertex, numbered by lowest vertex
    ncomponents: int
    normals: Optional[np.ndarray]        # (V, 3) float64, or None
    vertex_data: Optional[np.ndarray]    # (V, C) float64: the data of every vertex's first corner, or None
    level: Optional[np.ndarray]          # (S,) int32, passed through from a Contour
    element: Optional[np.ndarray]        # (S,) int32, passed through from a Contour or a Tessellation
    tol: float
    rounds: Tuple[int, int]              # labelling rounds of the vertex classes and of the components

    def degenerate(self) -> np.ndarray:
        """(S,) bool: the simplices with a repeated vertex."""
        c = self.cells
        if c.shape[1] == 2:
            return c[:, 0] == c[:, 1]
        return (c[:, 0] == c[:, 1]) | (c[:, 1] == c[:, 2]) | (c[:, 0] == c[:, 2])

    def _edge_keys(self) -> np.ndarray:
        """The packed keys `lo * V + hi` of the edges of every simplex that is not degenerate, one per (simplex, edge)."""
        c = self.cells[~self.degenerate()].astype(np.int64)
        if c.shape[1] == 2:
            a, b = c[:, 0], c[:, 1]
        else:
            a = np.concatenate([c[:, 0], c[:, 1], c[:, 2]])
            b = np.concatenate([c[:, 1], c[:, 2], c[:, 0]])
        return np.minimum(a, b) * max(self.vertices.shape[0], 1) + np.maximum(a, b)

    def edges(self):
        """`(edges (E, 2) int32, valence (E,) int64)`: the unique undirected edges `(lo, hi)` of the simplices that are not
        degenerate, in ascending `(lo, hi)` order, and how many of those simplices each edge belongs to."""
        keys, valence = np.unique(self._edge_keys(), return_counts=True)
        V = max(self.vertices.shape[0], 1)
        return np.stack([keys // V, keys % V], axis=1).astype(np.int32), valence.astype(np.int64)

    def vertex_valence(self) -> np.ndarray:
        """(V,) int64: the number of unique edges at every vertex."""
        e, _ = self.edges()
        return np.bincount(e.reshape(-1), minlength=self.vertices.shape[0]).astype(np.int64)

    def boundary_edges(self) -> np.ndarray:
        """(B, 2) int32.  Triangles: the edges that belong to exactly one triangle.  Segments: the edges with an end at
        which no other edge continues (the ends of an open curve)."""
        e, valence = self.edges()
        if self.cells.shape[1] == 3:
            return e[valence == 1]
        vv = self.vertex_valence()
        return e[(vv[e[:, 0]] == 1) | (vv[e[:, 1]] == 1)] if e.size else e

    def is_closed(self) -> bool:
        """Triangles: every edge belongs to exactly two triangles.  Segments: exactly two edges meet at every vertex.
        A mesh with no edge is not closed."""
        e, valence = self.edges()
        if e.shape[0] == 0:
            return False
        if self.cells.shape[1] == 3:
            return bool(np.all(valence == 2))
        return bool(np.all(self.vertex_valence() == 2))

    def euler_characteristic(self) -> np.ndarray:
        """(ncomponents,) int64: vertices - edges + triangles of every component, degenerate simplices left out."""
        n = self.ncomponents
        e, _ = self.edges()
        chi = np.bincount(self.component, minlength=n).astype(np.int64)
        chi -= np.bincount(self.component[e[:, 0]], minlength=n)
        if self.cells.shape[1] == 3:
            good = self.cells[~self.degenerate()]
            chi += np.bincount(self.component[good[:, 0]], minlength=n)
        return chi

    def save(self, path) -> None:
        """Write the mesh as ASCII Wavefront `.obj` (v / vn / l or f) or legacy ASCII `.vtk` POLYDATA (`vertex_data` and
        `component` as POINT_DATA, `level` as CELL_DATA), chosen by the suffix of `path`; coordinates with 17 significant
        digits.  A 2-D mesh is written with a third coordinate of 0.  Any other suffix raises `ValueError`."""
        suffix = os.path.splitext(str(path))[1].lower()
        if suffix not in (".obj", ".vtk"):
            raise ValueError(f"IndexedMesh.save: the suffix must be .obj or .vtk (got {str(path)!r})")
        P = self.vertices
        if P.shape[1] == 2:
            P = np.concatenate([P, np.zeros((P.shape[0], 1))], axis=1)
        V, (S, nv) = P.shape[0], self.cells.shape
        num = lambda row: " ".join("%.17g" % v for v in row)     # noqa: E731
        out = []
        if suffix == ".obj":
            out.append("# multigridbarrier weld: %d vertices, %d %s" % (V, S, "segments" if nv == 2 else "triangles"))
            out += ["v " + num(p) for p in P]
            if self.normals is not None:
                out += ["vn " + num(n) for n in self.normals]
            for c in self.cells + 1:
                if nv == 2:
                    out.append("l %d %d" % tuple(c))
                elif self.normals is not None:
                    out.append("f %d//%d %d//%d %d//%d" % (c[0], c[0], c[1], c[1], c[2], c[2]))
                else:
                    out.append("f %d %d %d" % tuple(c))
        else:
            out += ["# vtk DataFile Version 3.0", "multigridbarrier weld", "ASCII", "DATASET POLYDATA",
                    "POINTS %d double" % V]
            out += [num(p) for p in P]
            out.append("%s %d %d" % ("LINES" if nv == 2 else "POLYGONS", S, S * (nv + 1)))
            out += [("%d " % nv) + " ".join("%d" % v for v in c) for c in self.cells]
            if self.level is not None:
                out += ["CELL_DATA %d" % S, "SCALARS level int 1", "LOOKUP_TABLE default"]
                out += ["%d" % v for v in self.level]
            out += ["POINT_DATA %d" % V, "SCALARS component int 1", "LOOKUP_TABLE default"]
            out += ["%d" % v for v in self.component]
            if self.vertex_data is not None:
                for j in range(self.vertex_data.shape[1]):
                    out += ["SCALARS data%d double 1" % j, "LOOKUP_TABLE default"]
                    out += ["%.17g" % v for v in self.vertex_data[:, j]]
            if self.normals is not None:
                out.append("NORMALS normals double")
                out += [num(n) for n in self.normals]
        with open(path, "w") as fh:
            fh.write("\n".join(out) + "\n")


def _stream_segments(sl: Streamlines) -> np.ndarray:
    """(S, 2, d): the consecutive points of every line of a `Streamlines`, line by line."""
    d = int(np.asarray(sl.points).shape[-1])
    parts = [np.stack([ln[:-1], ln[1:]], axis=1) for ln in sl.lines() if ln.shape[0] >= 2]
    return np.concatenate(parts) if parts else np.zeros((0, 2, d))


def _check(soup, tol, normals, group, data):
    """Every argument check of `weld()`; returns what the device call needs."""
    level = element = None
    if isinstance(soup, Contour):
        P, level, element = soup.points, soup.level, soup.element
        if group is None:
            group = soup.level
        if data is None:
            data = soup.carried
    elif isinstance(soup, Tessellation):
        P, element = soup.points, soup.element
        if data is None:
            data = soup.values
    elif isinstance(soup, Streamlines):
        P = _stream_segments(soup)
    else:
        try:
            P = np.asarray(soup, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weld: the soup must be a Contour, a Tessellation, a Streamlines or an (S, nv, e) array (got "
                             f"{type(soup).__name__})") from None
    P = np.ascontiguousarray(P, dtype=np.float64)
    if P.ndim != 3:
        raise ValueError(f"weld: the soup must be (S, nv, e): simplex, corner, coordinate (got shape {P.shape})")
    S, nv, e = (int(v) for v in P.shape)
    if nv not in (2, 3):
        raise ValueError(f"weld: nv must be 2 (segments) or 3 (triangles) (got {nv})")
    if e not in (2, 3):
        raise ValueError(f"weld: e must be 2 or 3 (got {e})")
    if S * nv >= 2 ** 31:
        raise ValueError("weld: S x nv corners exceed 32-bit indexing (M >= 2^31)")
    if normals and (nv, e) != (3, 3):
        raise ValueError("weld: normals need triangles in R^3 (nv = 3, e = 3)")
    if tol is not None:
        if isinstance(tol, bool) or not isinstance(tol, (int, float, np.integer, np.floating)):
            raise ValueError(f"weld: tol must be a number or None (got {tol!r})")
        tol = float(tol)
        if not (np.isfinite(tol) and tol >= 0.0):
            raise ValueError(f"weld: tol must be finite and >= 0 (got {tol!r})")
    G = None
    if group is not None:
        G = np.asarray(group)
        if G.shape != (S,) or not np.issubdtype(G.dtype, np.integer):
            raise ValueError(f"weld: group must be ({S},) integers, one per simplex (got shape {G.shape}, dtype {G.dtype})")
        if G.size and (G.min() < -2 ** 31 or G.max() >= 2 ** 31):
            raise ValueError("weld: group must fit 32-bit integers")
        G = np.ascontiguousarray(G, dtype=np.int32)
    D = None
    if data is not None:
        D = np.asarray(data, dtype=np.float64)
        if D.shape == (S, nv):
            D = D[..., None]
        if D.ndim != 3 or D.shape[:2] != (S, nv):
            raise ValueError(f"weld: data must be ({S}, {nv}) or ({S}, {nv}, C), one row per corner (got shape {D.shape})")
    if not np.all(np.isfinite(P)):
        raise ValueError("weld: a corner has a non-finite coordinate")
    if tol is None:
        flat = P.reshape(-1, e)
        ext_max = float(np.max(flat.max(axis=0) - flat.min(axis=0))) if S else 0.0
        tol = DEFAULT_TOL_REL * ext_max
    return P, S, nv, e, float(tol), G, D, level, element


def weld(soup, tol: Optional[float] = None, normals: bool = False, group=None, data=None,
         device_id: int = 0) -> IndexedMesh:
    """Weld a simplex soup into an indexed mesh.

    `soup` is a `Contour` (its `level` is the group and its `carried` the data, unless given; `level` and `element` are
    passed through), a `Tessellation` (its `values` are the data), a `Streamlines` (the consecutive points of every line)
    or an `(S, nv, e)` float array with `nv` in {2, 3} (segments, triangles) and `e` in {2, 3}.  The `M = S nv` corners
    are numbered simplex-major.

    - Two corners are linked iff their simplices have the same `group` (`(S,)` integers; one group when None) and
      `fabs(x_a - y_a) <= tol` on every axis.  A vertex is a connected component of the link graph, so chains weld.
    - Vertices are numbered by their lowest corner, `first_corner[v]`, and `vertices[v]` is that corner's position:
      nothing is averaged.  `cells[s, j]` is the vertex of corner `j` of simplex `s`; a simplex with two corners in one
      vertex is kept (`degenerate()` finds it), so `cells` stays aligned with the soup.
    - `component[v]` is the connected component of vertex `v` in the graph of the simplex edges, numbered by lowest vertex.
    - `normals=True` (triangles in R^3 only): the normal of a vertex is the sum of `cross(p1 - p0, p2 - p0)` over the
      triangles of its corners in ascending corner order, divided by its length; zeros when the length is 0 or not finite.
    - `data` is `(S, nv)` or `(S, nv, C)`: `vertex_data[v]` is the row of the vertex's first corner, gathered on the host.

    `tol=None` means `2**-27` of the largest extent of the soup (copies of a vertex lie some 1e-16 of the extent apart and
    distinct vertices of the level sets some 1e-4); a `tol` given explicitly is used as it is, and `tol = 0` welds equal
    coordinates (`0.0` and `-0.0` are equal).  The corners are sorted into a grid of cell side
    `max(tol, extent / 2**20)`; more than 1024 corners in one cell (a tolerance far too large, or a soup that is one
    point) raise `ValueError` before any pair is tested.  Every other refusal is a `ValueError` raised before any device
    work.  An empty soup returns an empty mesh without touching the device.  Two calls return bitwise equal arrays.
    """
    P, S, nv, e, tol, G, D, level, element = _check(soup, tol, normals, group, data)
    if S == 0:
        return IndexedMesh(np.zeros((0, e)), np.zeros((0, nv), dtype=np.int32), np.zeros(0, dtype=np.int32),
                           np.zeros(0, dtype=np.int32), 0, np.zeros((0, 3)) if normals else None,
                           None if D is None else np.zeros((0, D.shape[2])), level, element, tol, (0, 0))
    from .device import ERR_INVALID, HipContext, MGBHipError, _check as _status, _ptr
    ip = C.POINTER(C.c_int32)
    ctx = HipContext(device_id)
    handle = None
    try:
        h = C.c_void_p()
        nV, nC = C.c_int64(0), C.c_int64(0)
        try:
            _status(ctx.lib, ctx.lib.mgbhip_weld_create(ctx.handle, S, nv, e, _ptr(P), None if G is None else G.ctypes.data_as(ip),
                                                        tol, 1 if normals else 0, C.byref(h), C.byref(nV), C.byref(nC)))
        except MGBHipError as err:
            if err.status == ERR_INVALID:
                raise ValueError(str(err)) from None
            raise
        handle = h
        V, ncomp = int(nV.value), int(nC.value)
        cells = np.empty((S, nv), dtype=np.int32)
        first = np.empty(V, dtype=np.int32)
        comp = np.empty(V, dtype=np.int32)
        nrm = np.empty((V, 3)) if normals else None
        _status(ctx.lib, ctx.lib.mgbhip_weld_fetch(handle, cells.ctypes.data_as(ip), first.ctypes.data_as(ip),
                                                   comp.ctypes.data_as(ip), _ptr(nrm)))
        r0, r1 = C.c_int32(0), C.c_int32(0)
        _status(ctx.lib, ctx.lib.mgbhip_weld_rounds(handle, C.byref(r0), C.byref(r1)))
    finally:
        if handle is not None:
            ctx.lib.mgbhip_weld_destroy(handle)
        ctx.close()
    vertices = P.reshape(-1, e)[first]
    vdata = None if D is None else D.reshape(S * nv, -1)[first]
    return IndexedMesh(vertices, cells, first, comp, ncomp, nrm, vdata, level, element, tol, (int(r0.value), int(r1.value)))
