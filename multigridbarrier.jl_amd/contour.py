"""Level sets of a solution: `isocontour(geom, z, levels)` gives level curves (2-D) and isosurfaces (3-D) as a simplex soup;
`tessellate(geom, fields)` gives the lattice triangles of a 2-D mesh themselves, flat or a `fem2d` surface in R^3.

The reference draws isosurfaces and slices of `fem3d` solutions by contouring a VTK grid with PyVista on the CPU
(ext/MultiGridBarrierPyPlotExt/plot3d.jl:85-150).  Here the level set is cut straight from the elements on the device in
one call of `mgbhip_contour_create` (csrc/contour.hip); the host only checks arguments and builds the small basis tables
`interpolate()` also builds.  Arguments are checked before any device work.  Nothing here plots: the result is a plain
list of segments or triangles that any plotting or measuring code can consume.

The reference also draws a solution on a `fem2d` surface in R^3 by cutting every Q_k quad into linear cells over its
tensor nodes (ext/MultiGridBarrierPyPlotExt/plot3d.jl:182-256).  `tessellate()` is that cutting on the device
(`mgbhip_tessellate_create`, the same file and the same lattice as the level sets), and `isocontour()` accepts such a
surface: the level curves are then segments in R^3.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .interpolate import MAX_DEGREE, P1, P2, P2C, QK, _c_f64, _plan
from .multigrid import Geometry
from .tensorfem import TensorFEM, _tf_nodes

MAX_CARRY = 4           # csrc/contour.hpp CONTOUR_MAX_FIELDS - 1
MAX_REFINE = {2: 16, 3: 8}   # csrc/contour.hpp CONTOUR_MAX_REFINE_2D / _3D


@dataclass
class Contour:
    """The simplex soup `isocontour()` returns: `S` simplices of `d` vertices each (segments for d = 2, triangles for
    d = 3) in `e` coordinates (`e = d`, or 3 for the level curves of a `fem2d` surface in R^3), unindexed (a vertex
    shared by two simplices appears in both, with the same bits)."""
    points: np.ndarray               # (S, d, e) float64: simplex, vertex, physical coordinate
    level: np.ndarray                # (S,) int32: index into `levels`
    element: np.ndarray              # (S,) int32: the element the simplex was cut from
    carried: Optional[np.ndarray]    # (S, d, ncarry) float64, or None
    nlevels: int

    def measure(self) -> np.ndarray:
        """(nlevels,) float64: the total length (d = 2) or area (d = 3) of the simplices of each level, summed on the
        host from `points`."""
        P = self.points
        d = P.shape[1]
        if d == 2 and P.shape[2] == 2:
            m = np.hypot(P[:, 1, 0] - P[:, 0, 0], P[:, 1, 1] - P[:, 0, 1])
        elif d == 2:
            m = np.sqrt(np.sum((P[:, 1] - P[:, 0]) ** 2, axis=1))
        else:
            m = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)
        return np.bincount(self.level, weights=m, minlength=self.nlevels).astype(np.float64)


@dataclass
class Tessellation:
    """The triangle soup `tessellate()` returns: the `T` lattice triangles of a 2-D mesh in `e` coordinates, unindexed,
    element by element (`T / N` each), the vertices of a triangle in ascending lattice index."""
    points: np.ndarray               # (T, 3, e) float64: triangle, vertex, physical coordinate
    element: np.ndarray              # (T,) int32: the element the triangle lies in
    values: Optional[np.ndarray]     # (T, 3, nfield) float64: the fields at the vertices, or None

    def measure(self) -> float:
        """The total area of the triangles, summed on the host from `points`: half the norm of the cross product for
        `e = 3`, half the absolute 2 x 2 determinant for `e = 2`."""
        P = self.points
        a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        if P.shape[2] == 3:
            m = 0.5 * np.linalg.norm(np.cross(a, b), axis=1)
        else:
            m = 0.5 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])
        return float(np.sum(m))


def _contour_plan(geom: Geometry, who: str = "isocontour", surfaces_only: bool = False):
    """`interpolate._plan` restricted to the families that have level sets, plus the `fem2d` surface in R^3, which
    `_plan` refuses because `interpolate` does; ValueError names the family otherwise.  Returns
    (family, name, d, e, k, p, N, node coordinates (p*N, e), table)."""
    disc = geom.discretization
    if isinstance(disc, TensorFEM) and disc.e != disc.d:
        if not (disc.d == 2 and disc.e == 3):
            raise ValueError(f"{who}: fem{disc.d}d embedded in {disc.e} dimensions (a manifold) is not supported")
        if not 1 <= disc.k <= MAX_DEGREE:
            raise ValueError(f"{who}: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
        p, N, _ = geom.x.shape
        # what `_plan` returns for a flat fem2d (QK, the k + 1 reference nodes `_tf_nodes(k)` as the table), with e = 3
        return QK, "fem2d", 2, 3, disc.k, p, N, geom.xflat, _tf_nodes(disc.k)
    family, name, d, k, p, N, xnodes, table = _plan(geom)
    if surfaces_only:
        if family not in (QK, P1, P2, P2C) or d != 2:
            raise ValueError(f"{who}: {name} geometries are not supported (fem2d, flat or a surface in R^3, fem2d_P1 and "
                             "fem2d_P2 are)")
    elif family not in (QK, P1, P2, P2C):
        raise ValueError(f"{who}: {name} geometries are not supported (fem2d, fem3d, fem2d_P1 and fem2d_P2 are)")
    return family, name, d, d, k, p, N, xnodes, table


def default_refine(family: int, k: int) -> int:
    """The lattice `isocontour()` uses when `refine` is None: k for Q_k, 1 for P1, 2 for P2 (straight or curved)."""
    return k if family == QK else (1 if family == P1 else 2)


def _check(geom: Geometry, z, levels, refine, carry):
    """Every argument check of `isocontour()`; returns what the device call needs."""
    family, name, d, e, k, p, N, xnodes, table = _contour_plan(geom)
    if N == 0:
        raise ValueError(f"isocontour: the {name} geometry has no elements")
    Z = np.asarray(z, dtype=np.float64)
    if Z.ndim != 1 or Z.shape[0] != p * N:
        raise ValueError(f"isocontour: z must be a vector of {p * N} values for this {name} geometry (got shape {Z.shape})")
    fields = [Z.reshape(-1, 1)]
    ncarry = 0
    if carry is not None:
        Cr = np.asarray(carry, dtype=np.float64)
        if Cr.ndim not in (1, 2) or Cr.shape[0] != p * N:
            raise ValueError(f"isocontour: carry must be ({p * N},) or ({p * N}, ncarry) (got shape {Cr.shape})")
        Cr = Cr.reshape(p * N, -1)
        ncarry = Cr.shape[1]
        if not 1 <= ncarry <= MAX_CARRY:
            raise ValueError(f"isocontour: carry has {ncarry} columns; 1..{MAX_CARRY} are supported")
        fields.append(Cr)
    lev = np.asarray(levels, dtype=np.float64)
    if lev.ndim > 1:
        raise ValueError(f"isocontour: levels must be a scalar or a 1-D array (got {lev.ndim} dimensions)")
    lev = lev.reshape(-1)
    if not np.all(np.isfinite(lev)):
        raise ValueError("isocontour: every level must be finite")
    if refine is None:
        refine = default_refine(family, k)
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)):
        raise ValueError(f"isocontour: refine must be an integer (got {refine!r})")
    if not 1 <= refine <= MAX_REFINE[d]:
        raise ValueError(f"isocontour: refine = {refine} is outside 1..{MAX_REFINE[d]} for {d}-D elements")
    if not np.all(np.isfinite(xnodes)):
        raise ValueError(f"isocontour: the {name} mesh has non-finite node coordinates")
    F = np.concatenate(fields, axis=1)
    return family, d, e, k, p, N, xnodes, table, F, ncarry, lev, int(refine)


def isocontour(geom: Geometry, z, levels, refine: Optional[int] = None, carry=None, device_id: int = 0) -> Contour:
    """The level sets `{z = c}` for every `c` in `levels` of the element-space function with broken-basis values `z`.

    `z` is `(p*N,)` in `geom.xflat` row order (a column of `sol.z`), as for `interpolate()`.  `levels` is a scalar or a
    1-D array of finite values; duplicates are separate levels.  `carry` is `(p*N,)` or `(p*N, ncarry)` with
    `ncarry <= 4`: further element-space functions that are interpolated to every vertex of the result
    (`Contour.carried`); each carried column is bitwise what a call with that column alone returns.

    Supported: `fem2d` and `fem3d` (Q_k, `1 <= k <= 8`, curved elements included), `fem2d_P1`, `fem2d_P2` (with or
    without the bubble; curved elements when built with `curved=True`: the lattice positions are sums over all the
    element's nodes, as for Q_k), and `fem2d` surfaces in R^3 (`fem2d(K=..., ambient=3)`): their level curves
    are segments in R^3, `points` is `(S, 2, 3)`, and every coordinate is formed like the two of a flat mesh, so a
    surface whose third coordinate is `0.0` everywhere returns the bits of the flat call.  `fem1d` (also as a curve in
    R^2 / R^3) and the spectral families raise `ValueError`.

    The algorithm (the same on the device and in the NumPy restatement the tests compare it with):

    1. Every element is sampled on a uniform reference lattice: `refine + 1` equispaced points per axis of `[-1, 1]`
       for Q_k (axis 0 fastest), the barycentric lattice of the `refine`-fold uniform subdivision for P1 / P2.  The
       default is `refine = k` for Q_k, 1 for P1, 2 for P2; allowed are 1..16 in 2-D and 1..8 in 3-D.  The element's own
       basis gives the value of `z`, of the carried fields and the physical position (isoparametric for Q_k) there.
    2. A lattice square is split into two triangles along the diagonal from corner `(i, j)` to `(i+1, j+1)`; P1 / P2 use
       the `refine**2` triangles of the subdivision; a lattice cube is split into the six Kuhn tetrahedra around the
       diagonal `(i, j, k)`-`(i+1, j+1, k+1)`.  There are no case tables and no ambiguous cases.
    3. For a level `c` a vertex with value `>= c` is above.  A simplex with all vertices on one side, or with a
       non-finite vertex value, emits nothing; a triangle emits one segment; a tetrahedron one triangle (1-3 split) or
       two (2-2 split).  A crossing of lattice edge `(a, b)`, `a` the endpoint of lower lattice index, is at
       `t = (c - v_a) / (v_b - v_a)`, `x = x_a + t (x_b - x_a)`, so both simplices that share an edge compute the same
       bits.  The vertices of an emitted simplex are in ascending order of their edges' `(a, b)`.
    4. The order of the result is: element, lattice cell, simplex of the cell, level index, triangle of a 2-2 split.  It
       is produced by a count pass, a scan and an emit pass, not by atomics: two calls return bitwise equal arrays.

    Inside an element the soup is watertight (neighbouring simplices share their vertices bit for bit).  In 2-D that also
    holds across elements whose shared edge carries the same lattice from both sides.  In 3-D continuity across faces of
    different elements is not promised: neighbouring elements may orient the diagonals of a shared face differently.

    A slice through a 3-D solution is the isosurface of a coordinate function with the solution carried along:
    `isocontour(geom, geom.xflat[:, 0], [0.25], carry=u)` returns the plane `x = 0.25` in `points` and `u` on it in
    `carried[..., 0]`.

    A call with no levels returns an empty result without touching the device.
    """
    family, d, e, k, p, N, xnodes, table, F, ncarry, lev, refine = _check(geom, z, levels, refine, carry)
    nlev = int(lev.shape[0])
    S = 0
    ctx = handle = None
    try:
        if nlev:
            from .device import HipContext, _check as _status, _ptr
            F, lev, xnodes, table = _c_f64(F), _c_f64(lev), _c_f64(xnodes), _c_f64(table)
            ctx = HipContext(device_id)
            handle = C.c_void_p()
            n = C.c_int64(0)
            try:
                _status(ctx.lib, ctx.lib.mgbhip_contour_create_embedded(
                    ctx.handle, family, d, e, k, p, N, _ptr(xnodes), _ptr(table), 1 + ncarry, _ptr(F), nlev, _ptr(lev),
                    refine, C.byref(handle), C.byref(n)))
            except Exception:
                handle = None
                raise
            S = int(n.value)
        points = np.empty((S, d, e))
        level = np.empty(S, dtype=np.int32)
        element = np.empty(S, dtype=np.int32)
        carried = np.empty((S, d, ncarry)) if ncarry else None
        if S:
            ip = C.POINTER(C.c_int32)
            _status(ctx.lib, ctx.lib.mgbhip_contour_fetch(handle, _ptr(points), level.ctypes.data_as(ip),
                                                          element.ctypes.data_as(ip), _ptr(carried)))
    finally:
        if handle is not None:
            ctx.lib.mgbhip_contour_destroy(handle)
        if ctx is not None:
            ctx.close()
    return Contour(points, level, element, carried, nlev)


def _check_tessellate(geom: Geometry, fields, refine):
    """Every argument check of `tessellate()`; returns what the device call needs."""
    who = "tessellate"
    family, name, d, e, k, p, N, xnodes, table = _contour_plan(geom, who, surfaces_only=True)
    if N == 0:
        raise ValueError(f"{who}: the {name} geometry has no elements")
    F = None
    if fields is not None:
        F = np.asarray(fields, dtype=np.float64)
        if F.ndim not in (1, 2) or F.shape[0] != p * N:
            raise ValueError(f"{who}: fields must be ({p * N},) or ({p * N}, nfield) for this {name} geometry (got shape "
                             f"{F.shape})")
        F = F.reshape(p * N, -1)
        if not 1 <= F.shape[1] <= MAX_CARRY + 1:
            raise ValueError(f"{who}: fields has {F.shape[1]} columns; 1..{MAX_CARRY + 1} are supported")
    if refine is None:
        refine = default_refine(family, k)
    if isinstance(refine, bool) or not isinstance(refine, (int, np.integer)):
        raise ValueError(f"{who}: refine must be an integer (got {refine!r})")
    if not 1 <= refine <= MAX_REFINE[2]:
        raise ValueError(f"{who}: refine = {refine} is outside 1..{MAX_REFINE[2]} for 2-D elements")
    if not np.all(np.isfinite(xnodes)):
        raise ValueError(f"{who}: the {name} mesh has non-finite node coordinates")
    ntri = (2 if family == QK else 1) * int(refine) ** 2
    if N * ntri * 3 > 2 ** 31 - 1:
        raise ValueError(f"{who}: T = {N * ntri} triangles have more than 2^31 - 1 vertices: use a smaller refine")
    return family, d, e, k, p, N, xnodes, table, F, int(refine)


def tessellate(geom: Geometry, fields=None, refine: Optional[int] = None, device_id: int = 0) -> Tessellation:
    """Every lattice triangle of a 2-D mesh, with the element-space functions `fields` at its vertices.

    The restatement of how the reference draws a solution on a surface
    (ext/MultiGridBarrierPyPlotExt/plot3d.jl:182-256: every Q_k quad cut into linear cells over its tensor nodes),
    on the device.  `fields` is `(p*N,)` or `(p*N, nfield)` with `nfield <= 5`, in `geom.xflat` row order, or None.

    Supported: `fem2d` (flat, or a surface in R^3: `fem2d(K=..., ambient=3)`), `fem2d_P1`, `fem2d_P2` (curved
    elements when built with `curved=True`).  Everything else raises `ValueError` naming the family.

    The lattice and its triangles are those of `isocontour()` (steps 1 and 2 there; the same device code forms them):
    `refine + 1` equispaced points per axis for Q_k, the barycentric lattice for P1 / P2, the position and every field a
    sum of p products in ascending node order; per lattice square the two triangles on the diagonal `(i, j)`-`(i+1,
    j+1)`, or the `refine**2` triangles of the subdivision.  The default `refine` is that of `isocontour()` (k for Q_k,
    1 for P1, 2 for P2), which reproduces the element's own nodes; allowed are 1..16.  Element `n` owns the triangles
    `n * ntri .. (n + 1) * ntri - 1` (`ntri = 2 refine**2` for Q_k, `refine**2` for P1 / P2) in the order `isocontour()`
    walks them, each with its vertices in ascending lattice index.  `T` follows from `N` and `refine`, so there is one
    launch, no count pass and no atomics: two calls return bitwise equal arrays.  Every level-curve vertex of
    `isocontour()` with the same `refine` lies on an edge of a triangle of the same element, bit for bit.
    """
    family, d, e, k, p, N, xnodes, table, F, refine = _check_tessellate(geom, fields, refine)
    nfield = 0 if F is None else int(F.shape[1])
    from .device import HipContext, _check as _status, _ptr
    xnodes, table = _c_f64(xnodes), _c_f64(table)
    F = None if F is None else _c_f64(F)
    ctx = HipContext(device_id)
    handle = C.c_void_p()
    n = C.c_int64(0)
    try:
        try:
            _status(ctx.lib, ctx.lib.mgbhip_tessellate_create(
                ctx.handle, family, d, e, k, p, N, _ptr(xnodes), _ptr(table), nfield, _ptr(F), refine, C.byref(handle),
                C.byref(n)))
        except Exception:
            handle = None
            raise
        T = int(n.value)
        points = np.empty((T, 3, e))
        element = np.empty(T, dtype=np.int32)
        values = np.empty((T, 3, nfield)) if nfield else None
        _status(ctx.lib, ctx.lib.mgbhip_tessellate_fetch(handle, _ptr(points), element.ctypes.data_as(C.POINTER(C.c_int32)),
                                                         _ptr(values)))
    finally:
        if handle is not None:
            ctx.lib.mgbhip_tessellate_destroy(handle)
        ctx.close()
    return Tessellation(points, element, values)
