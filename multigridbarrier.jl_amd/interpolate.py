"""Point evaluation of a solution: `interpolate(geom, z, t)` (reference: src/utils.jl:16-58).

The reference covers 1-D Q_k FEM (src/TensorFEM.jl:957-1014), `spectral1d` (src/spectral1d.jl:140-170) and `spectral2d`
(src/spectral2d.jl:85-125); this module also covers the 2-D and 3-D element families (Q_k, P1, P2), which the reference
does not.  Every evaluation runs on the device in one call of `mgbhip_interpolate` (csrc/interpolate.hip), or of
`mgbhip_interpolate_grad` when the gradient at the points is wanted as well (`gradient=True`); the host
only checks arguments, builds the small basis tables and, for the spectral families, forms the Chebyshev coefficients
exactly as the reference does (`evaluation(x, n) \\ z`).  Arguments are checked before any device work.

`PointLocator(geom, t)` does the part of that call that does not depend on `z` once (`mgbhip_locator_create`) and keeps
the result on the device; its `evaluate(z)` is bitwise `interpolate(geom, z, t)` and shares the argument checks, the
coefficient solve and the result shapes with it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fem2d_p1, fem2d_p2
from .fem2d_p1 import FEM2D_P1
from .fem2d_p2 import FEM2D_P2
from ._handle import DeviceObject
from .multigrid import Geometry
from .spectral import SPECTRAL1D, SPECTRAL2D, evaluation
from .tensorfem import TensorFEM, _tf_nodes

# include/mgbhip.h MGBHIP_INTERP_*
FEM1D, QK, P1, P2, SPECTRAL_1D, SPECTRAL_2D = range(1, 7)
P2C = 7                 # MGBHIP_INTERP_P2C: fem2d_P2 with curved elements (`fem2d_P2(..., curved=True)`)
MAX_DEGREE = 8          # csrc/interpolate.hpp INTERP_MAX_DEGREE


def _c_f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)


def _spectral_basis(family: int, geom: Geometry):
    """The Chebyshev evaluation matrix the coefficients are solved against: (V, n), or None for the FEM families."""
    if family == SPECTRAL_1D:
        x = geom.xflat[:, 0]
        return evaluation(x, len(x)), len(x)
    if family == SPECTRAL_2D:
        n = geom.discretization.n
        return evaluation(geom.xflat[:n, 0], n), n
    return None


def _spectral_coefficients(family: int, basis, Z: np.ndarray) -> np.ndarray:
    """What the device evaluates: Z itself for the FEM families, the Chebyshev coefficients for the spectral ones.

    spectral1d: c = evaluation(x, n) \\ z, column by column (src/spectral1d.jl:140-150).  spectral2d:
    C = V \\ reshape(z, n, n) / V', column by column (src/spectral2d.jl:85-92); row i*n + j of the result is C[i, j]."""
    if basis is None:
        return Z
    V, n = basis
    if family == SPECTRAL_1D:
        return np.stack([np.linalg.solve(V, Z[:, j]) for j in range(Z.shape[1])], axis=1)
    cols = []
    for j in range(Z.shape[1]):
        Y = np.linalg.solve(V, Z[:, j].reshape(n, n, order="F"))
        Cm = np.linalg.solve(V, Y.T).T                 # Y / V'  =  (V \\ Y')'
        cols.append(Cm.reshape(-1))
    return np.stack(cols, axis=1)


def _spectral1d_coefficients(geom: Geometry, Z: np.ndarray) -> np.ndarray:
    return _spectral_coefficients(SPECTRAL_1D, _spectral_basis(SPECTRAL_1D, geom), Z)


def _spectral2d_coefficients(geom: Geometry, Z: np.ndarray) -> np.ndarray:
    return _spectral_coefficients(SPECTRAL_2D, _spectral_basis(SPECTRAL_2D, geom), Z)


def _check_p2_straight(x: np.ndarray, bubble: bool) -> None:
    RK = fem2d_p2.reference_triangle(bubble)["K"]
    straight = np.einsum("vc,ced->ved", RK, x[[0, 2, 4], :, :])
    tol = 1e-12 * max(1.0, float(np.abs(x).max()))
    if not np.all(np.abs(straight - x) <= tol):
        raise ValueError("fem2d_P2 interpolation needs straight elements: every edge node at its edge's midpoint"
                         + (" and the bubble node at the centroid" if bubble else ""))


def _plan(geom: Geometry):
    """(family, name, d, k, p, N, node coordinates or None, table or None) of a geometry; ValueError if unsupported."""
    disc = geom.discretization
    if isinstance(disc, TensorFEM):
        if disc.e != disc.d:
            raise ValueError(f"interpolate: embedded manifolds (TensorFEM with d = {disc.d} < e = {disc.e}) are not "
                             "supported")
        if not 1 <= disc.k <= MAX_DEGREE:
            raise ValueError(f"interpolate: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
        p, N, d = geom.x.shape
        return (FEM1D if d == 1 else QK), f"fem{d}d", d, disc.k, p, N, geom.xflat, _tf_nodes(disc.k)
    if isinstance(disc, FEM2D_P1):
        p, N, _ = geom.x.shape
        return P1, "fem2d_P1", 2, 1, p, N, geom.xflat, fem2d_p1.basis_coefficient_table()
    if isinstance(disc, FEM2D_P2):
        p, N, _ = geom.x.shape
        family = P2                # straight elements take the affine path whatever the flag says
        try:
            _check_p2_straight(geom.x, p == 7)
        except ValueError as err:
            if not disc.curved:
                raise ValueError(f"{err} (build the geometry with fem2d_P2(..., curved=True) to evaluate on curved "
                                 "elements)") from None
            family = P2C
        return family, "fem2d_P2", 2, 2, p, N, geom.xflat, fem2d_p2.basis_coefficient_table(p == 7)
    if isinstance(disc, SPECTRAL1D):
        n = len(geom.w)
        return SPECTRAL_1D, "spectral1d", 1, n - 1, n, 1, None, None
    if isinstance(disc, SPECTRAL2D):
        n = disc.n
        return SPECTRAL_2D, "spectral2d", 2, n - 1, n * n, 1, None, None
    raise ValueError(f"interpolate: no method for {type(disc).__name__} geometries")


def _columns(name: str, p: int, N: int, z):
    """(Z as (p*N, ncomp), whether z was a vector); ValueError unless z is a vector or matrix of p*N rows."""
    Z = np.asarray(z, dtype=np.float64)
    if Z.ndim not in (1, 2):
        raise ValueError(f"interpolate: z must be a vector or a matrix (got {Z.ndim} dimensions)")
    single = Z.ndim == 1
    Z = Z.reshape(Z.shape[0], -1)
    if Z.shape[0] != p * N:
        raise ValueError(f"{name} interpolation needs {p * N} values (got {Z.shape[0]})")
    if Z.shape[1] < 1:
        raise ValueError("interpolate: z has no columns")
    return Z, single


def _points(name: str, d: int, N: int, xnodes, t):
    """(points as (M, d), scalar, shape of the leading axes); ValueError for a wrong shape or an unusable mesh."""
    if N == 0:
        raise ValueError(f"{name} interpolation needs at least one element")
    T = np.asarray(t, dtype=np.float64)
    if d == 1:
        scalar = T.ndim == 0
        shape = T.shape
        pts = T.reshape(-1, 1)
    else:
        if T.ndim == 1 and T.shape[0] == d:
            scalar, shape = True, ()
            pts = T.reshape(1, d)
        elif T.ndim == 2 and T.shape[1] == d:
            scalar, shape = False, (T.shape[0],)
            pts = T
        else:
            raise ValueError(f"{name} interpolation points must form an M-by-{d} array (got shape {T.shape})")
    if xnodes is not None and not np.all(np.isfinite(xnodes)):
        raise ValueError(f"{name} interpolation: the mesh has non-finite node coordinates")
    return pts, scalar, shape


def _shape_elements(elem: np.ndarray, scalar: bool, shape):
    return int(elem[0]) if scalar else elem.reshape(shape)


def _shape_values(out: np.ndarray, grad, d: int, single: bool, scalar: bool, shape):
    """(values, grads or None) in the shapes interpolate() documents, from out (M, ncomp) and grad (M, ncomp, d)."""
    ncomp = out.shape[1]
    vals = out[:, 0] if single else out
    if scalar:
        vals = vals[0] if single else vals[0].copy()
        if single:
            vals = float(vals)
    else:
        vals = vals.reshape(shape + (() if single else (ncomp,)))
    if grad is None:
        return vals, None
    g = grad[:, 0] if single else grad                       # (M, d) or (M, ncomp, d)
    if d == 1:
        g = g[..., 0]
    if scalar:
        g = g[0]
        g = float(g) if g.ndim == 0 else g.copy()
    else:
        g = g.reshape(shape + g.shape[1:])
    return vals, g


def interpolate(geom: Geometry, z, t, device_id: int = 0, return_element: bool = False, gradient: bool = False):
    """Evaluate the element-space function with broken-basis values `z` at the points `t`.

    `z` is `(p*N,)` in `geom.xflat` row order (a column of `sol.z`), or `(p*N, k)`: the result then has a trailing axis
    of `k`, each column bitwise what a 1-column call returns.  1-D geometries take a scalar `t` (scalar result) or an
    array (result of the same shape); 2-D and 3-D ones take `(M, d)` points (result `(M,)`) or one point `(d,)`
    (scalar).

    - fem1d: the reference's algorithm (src/TensorFEM.jl:967-1014), clamped outside the mesh: `t <= x[0]` gives the
      first value, `t >= x[-1]` the last (also for +-Inf); NaN gives NaN.
    - fem2d / fem3d (Q_k), fem2d_P1, fem2d_P2: the element map of the lowest-index element that contains the point
      (within a 1e-11 tolerance in reference coordinates) is inverted and the element's basis evaluated; a point
      outside the mesh, or with a NaN or Inf coordinate, gives NaN.  fem2d_P2 elements must be straight (every edge
      node at its edge's midpoint, the bubble at the centroid) unless the geometry was built with
      `fem2d_P2(..., curved=True)`: curved elements are then inverted by Newton over all their nodes, as for Q_k.
    - spectral1d / spectral2d: the Chebyshev interpolant of the reference, not clamped; a non-finite point gives NaN.

    With `return_element=True` the result is `(values, elements)`: the int32 element used per point (-1: none; the
    spectral families report 0).

    With `gradient=True` the result is `(values, grads)` or `(values, grads, elements)`: the gradient with respect to x
    at each point, evaluated on the device next to the value (`mgbhip_interpolate_grad`).  `grads` has the shape of
    `values` with the component axis (if any) followed by a trailing axis of length `d`; for 1-D geometries that axis
    is dropped, so `grads` has the shape of `values`.  The values are bitwise those of `gradient=False`.

    - fem2d / fem3d: `J^{-T} sum_i grad_xi phi_i z_i` with the Jacobian of the element map at the located reference
      point (curved elements included); fem2d_P1 / fem2d_P2: the basis differentiated in barycentric coordinates and
      mapped by the inverse transpose of the edge vectors, or, on curved fem2d_P2 elements, of the Jacobian
      `J[a][b] = sum_j dphi_j/dl_b x_j[a]` at the located barycentric pair.
    - fem1d: the derivative of the element's interpolant over `dx/dxi`.  Values are clamped outside the mesh, so the
      derivative there is 0.0; at `x[0]` and `x[-1]` it is the one-sided derivative of the end element; NaN gives NaN.
    - spectral1d / spectral2d: the derivative of the Chebyshev interpolant (finite at +-1); a non-finite point gives NaN.
    - A point whose value is NaN has NaN in every gradient entry.  The gradient of an element-space function is
      discontinuous across element faces: a point on a shared face (or node) reports the gradient of the lowest-index
      element that contains it, the same element its value comes from, which is what makes the result deterministic.
    """
    family, name, d, k, p, N, xnodes, table = _plan(geom)
    Z, single = _columns(name, p, N, z)
    pts, scalar, shape = _points(name, d, N, xnodes, t)
    Zd = _spectral_coefficients(family, _spectral_basis(family, geom), Z)
    M, ncomp = pts.shape[0], Z.shape[1]
    out = np.empty((M, ncomp))
    grad = np.empty((M, ncomp, d)) if gradient else None
    elem = np.empty(M, dtype=np.int32)
    if M:
        from .device import HipContext, _check, _ptr
        Zd, pts = _c_f64(Zd), _c_f64(pts)
        xnodes = None if xnodes is None else _c_f64(xnodes)
        table = None if table is None else _c_f64(table)
        ctx = HipContext(device_id)
        try:
            eptr = elem.ctypes.data_as(C.POINTER(C.c_int32))
            if gradient:
                _check(ctx.lib, ctx.lib.mgbhip_interpolate_grad(
                    ctx.handle, family, d, k, p, N, _ptr(xnodes), _ptr(table), ncomp, _ptr(Zd), M, _ptr(pts),
                    _ptr(out), _ptr(grad), eptr))
            else:
                _check(ctx.lib, ctx.lib.mgbhip_interpolate(
                    ctx.handle, family, d, k, p, N, _ptr(xnodes), _ptr(table), ncomp, _ptr(Zd), M, _ptr(pts),
                    _ptr(out), eptr))
        finally:
            ctx.close()
    vals, g = _shape_values(out, grad, d, single, scalar, shape)
    elem_out = _shape_elements(elem, scalar, shape)
    if not gradient:
        return (vals, elem_out) if return_element else vals
    return (vals, g, elem_out) if return_element else (vals, g)


class PointLocator(DeviceObject):
    """The points `t` located once in `geom`, for evaluating many `z` at them: `loc.evaluate(z)` is bitwise
    `interpolate(geom, z, t)`, `loc.evaluate(z, gradient=True)` bitwise `interpolate(geom, z, t, gradient=True)` and
    `loc.elements` the elements `return_element=True` reports.

    The constructor makes every check `interpolate()` makes on the geometry and the points, then runs the part of the
    work that does not depend on `z` (`mgbhip_locator_create`: location grid, points sorted by cell, element map
    inverted per point) and leaves each point's element and reference coordinates on the device.  `evaluate` uploads
    one `z`, runs the evaluation kernel and copies the result back.  The locator holds copies of what it needs: later
    changes to `t` or `geom.x` do not change its results.  Use it as a context manager or call `close()`; a locator of
    zero points needs no device and no library.
    """

    _closed_message = "PointLocator: the locator is closed"
    _destroy = "mgbhip_locator_destroy"

    def __init__(self, geom: Geometry, t, device_id: int = 0):
        self._family, self._name, self._d, k, self._p, self._N, xnodes, table = _plan(geom)
        pts, self._scalar, self._shape = _points(self._name, self._d, self._N, xnodes, t)
        self._basis = _spectral_basis(self._family, geom)
        self.n_points = int(pts.shape[0])
        if self.n_points:
            from .device import _ptr
            pts = _c_f64(pts)
            xnodes = None if xnodes is None else _c_f64(xnodes)
            table = None if table is None else _c_f64(table)
            self._create(device_id, "mgbhip_locator_create", self._family, self._d, k, self._p, self._N, _ptr(xnodes),
                         _ptr(table), self.n_points, _ptr(pts))

    @property
    def elements(self):
        """The int32 element of each point (-1: none; the spectral families report 0, and -1 for a non-finite point),
        shaped like the points' leading axes (one point given as `(d,)` or a scalar: an int), as
        `interpolate(..., return_element=True)` reports it."""
        self._open()
        elem = np.zeros(self.n_points, dtype=np.int32)
        if self.n_points:
            from .device import _check
            _check(self._ctx.lib, self._ctx.lib.mgbhip_locator_elements(
                self._handle, elem.ctypes.data_as(C.POINTER(C.c_int32))))
        return _shape_elements(elem, self._scalar, self._shape)

    def evaluate(self, z, gradient: bool = False):
        """`interpolate(geom, z, t)` at the located points, or `(values, grads)` with `gradient=True`; shapes, the vector /
        matrix rule for `z` and the errors are those of `interpolate()`."""
        self._open()
        Z, single = _columns(self._name, self._p, self._N, z)
        M, ncomp, d = self.n_points, Z.shape[1], self._d
        out = np.empty((M, ncomp))
        grad = np.empty((M, ncomp, d)) if gradient else None
        if M:
            from .device import _check, _ptr
            Zd = _c_f64(_spectral_coefficients(self._family, self._basis, Z))
            _check(self._ctx.lib, self._ctx.lib.mgbhip_locator_evaluate(
                self._handle, ncomp, _ptr(Zd), _ptr(out), _ptr(grad)))
        vals, g = _shape_values(out, grad, d, single, self._scalar, self._shape)
        return (vals, g) if gradient else vals
