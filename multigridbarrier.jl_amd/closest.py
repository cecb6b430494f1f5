"""Point evaluation on embedded curves and surfaces: `closest_point(geom, z, t)` and `ClosestPointLocator(geom, t)`.

`interpolate()` evaluates at points of a flat mesh (`d == e`).  On a `fem1d(K=..., ambient=2|3)` curve or a
`fem2d(K=..., ambient=3)` surface a query point of R^e is never exactly on the discrete geometry (a point of the true
sphere is O(h^(k+1)) off the Q_k sphere), so the point is first projected to the closest point of the mesh, its *foot*,
and the element function is evaluated there.  The reference has no counterpart.

Everything runs on the device (csrc/closest.hip, `mgbhip_closest_*`): a grid of element boxes padded by `max_distance`
gives every point its candidate elements, one lane per point projects it onto each candidate by a projected Newton
iteration and keeps the nearest foot, and `evaluate` sums the element basis at the stored reference coordinates.  The
host only checks arguments, before any device work.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._handle import DeviceObject
from .interpolate import MAX_DEGREE, _c_f64, _columns, _shape_elements, _shape_values
from .multigrid import Geometry
from .tensorfem import TensorFEM, _tf_nodes

BOX_PAD = 0.125                  # csrc/interp_device.hpp QK_BOX_PAD: the fraction the default max_distance uses


def _plan(geom: Geometry):
    """(name, d, e, k, p, N) of an embedded Q_k geometry; ValueError for everything else."""
    disc = geom.discretization
    if not isinstance(disc, TensorFEM):
        raise ValueError(f"closest_point: no method for {type(disc).__name__} geometries (embedded fem1d curves and "
                         "fem2d surfaces are supported)")
    if disc.d == disc.e:
        raise ValueError(f"closest_point: fem{disc.d}d with d = e = {disc.d} is a flat mesh, not an embedded manifold; "
                         "use interpolate()")
    if (disc.d, disc.e) not in ((1, 2), (1, 3), (2, 3)):
        raise ValueError(f"closest_point: TensorFEM with d = {disc.d}, e = {disc.e} is not supported")
    if not 1 <= disc.k <= MAX_DEGREE:
        raise ValueError(f"closest_point: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
    p, N, e = geom.x.shape
    name = f"fem{disc.d}d"
    if N == 0:
        raise ValueError(f"closest_point: the {name} geometry has no elements")
    if not np.all(np.isfinite(geom.x)):
        raise ValueError(f"closest_point: the {name} mesh has non-finite node coordinates")
    return name, disc.d, e, disc.k, p, N


def _points(e: int, t):
    """(points (M, e), scalar, shape of the leading axes)."""
    T = np.asarray(t, dtype=np.float64)
    if T.ndim == 1 and T.shape[0] == e:
        return T.reshape(1, e), True, ()
    if T.ndim == 2 and T.shape[1] == e:
        return T, False, (T.shape[0],)
    raise ValueError(f"closest_point: the points must form an M-by-{e} array (got shape {T.shape})")


def default_max_distance(geom: Geometry) -> float:
    """0.125 x the largest diagonal of an element's node box."""
    x = np.asarray(geom.x, dtype=np.float64)
    ext = x.max(axis=0) - x.min(axis=0)                               # (N, e)
    return float(BOX_PAD * np.sqrt((ext * ext).sum(axis=1)).max())


def _max_distance(geom: Geometry, max_distance) -> float:
    if max_distance is None:
        return default_max_distance(geom)
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float, np.integer, np.floating)):
        raise ValueError("closest_point: max_distance must be a number or None")
    md = float(max_distance)
    if not math.isfinite(md) or md < 0.0:
        raise ValueError(f"closest_point: max_distance = {md} must be finite and >= 0")
    return md


class ClosestPointLocator(DeviceObject):
    """The points `t` (`(M, e)` or `(e,)`) projected once onto the embedded curve or surface `geom`, for evaluating many
    `z` at their feet.

    The foot of a point is the point of the whole mesh closest to it, among points within `max_distance` (default:
    0.125 x the largest diagonal of an element's node box, see `max_distance`); a point with no foot that near, or with a
    non-finite coordinate, has element -1 and NaN everywhere.  Per candidate element the squared distance is minimised
    over [-1, 1]^d by a projected Newton iteration from the element's node nearest to the point (at most 64 iterations;
    a candidate that does not converge competes with the distance at its last iterate, and `converged` tells whether the
    winner did).  Candidates are visited in ascending element index and a later one wins only on a strictly smaller
    distance, so a point equally near two elements reports the lower one.

    `elements` `(M,)` int32, `xi` `(M, d)` in [-1, 1]^d (exactly +-1 on an axis the foot is clamped on), `points` `(M, e)`
    the feet, `distances` `(M,)`, `converged` `(M,)` bool; one point given as `(e,)` drops the leading axis.  The locator
    holds copies of what it needs.  Use it as a context manager or call `close()`; a locator of zero points needs no
    device and no library.
    """

    _closed_message = "ClosestPointLocator: the locator is closed"
    _destroy = "mgbhip_closest_destroy"

    def __init__(self, geom: Geometry, t, max_distance=None, device_id: int = 0):
        self._name, self._d, self._e, k, self._p, self._N = _plan(geom)
        pts, self._scalar, self._shape = _points(self._e, t)
        self.max_distance = _max_distance(geom, max_distance)
        self.n_points = int(pts.shape[0])
        self._fetched = None
        if self.n_points:
            from .device import _ptr
            pts, x, nodes = _c_f64(pts), _c_f64(geom.xflat), _c_f64(_tf_nodes(k))
            self._create(device_id, "mgbhip_closest_create", self._d, self._e, k, self._N, _ptr(x), _ptr(nodes),
                         self.n_points, _ptr(pts), C.c_double(self.max_distance))

    def _fetch(self):
        self._open()
        if self._fetched is None:
            M = self.n_points
            elem, flag = np.full(M, -1, dtype=np.int32), np.zeros(M, dtype=np.int32)
            xi, foot, dist = np.full((M, self._d), np.nan), np.full((M, self._e), np.nan), np.full(M, np.nan)
            if M:
                from .device import _check, _ptr
                ip = C.POINTER(C.c_int32)
                _check(self._ctx.lib, self._ctx.lib.mgbhip_closest_fetch(
                    self._handle, elem.ctypes.data_as(ip), _ptr(xi), _ptr(foot), _ptr(dist), flag.ctypes.data_as(ip)))
            self._fetched = (elem, xi, foot, dist, flag != 0)
        return self._fetched

    def _lead(self, a):
        return a[0].copy() if self._scalar else a.copy()

    @property
    def elements(self):
        """The int32 element of each foot (-1: none), shaped like the points' leading axes (one point: an int)."""
        return _shape_elements(self._fetch()[0].copy(), self._scalar, self._shape)

    @property
    def xi(self):
        """`(M, d)`: the reference coordinates of the feet (NaN where `elements` is -1)."""
        return self._lead(self._fetch()[1])

    @property
    def points(self):
        """`(M, e)`: the feet `x_elem(xi)` (NaN where `elements` is -1)."""
        return self._lead(self._fetch()[2])

    @property
    def distances(self):
        """`(M,)`: `|foot - t|` (NaN where `elements` is -1)."""
        d = self._fetch()[3]
        return float(d[0]) if self._scalar else d.copy()

    @property
    def converged(self):
        """`(M,)` bool: the winning candidate's iteration met its stopping test (False where `elements` is -1)."""
        c = self._fetch()[4]
        return bool(c[0]) if self._scalar else c.copy()

    def evaluate(self, z, gradient: bool = False):
        """The element function with broken-basis values `z` (`(p*N,)` or `(p*N, ncomp)`, as for `interpolate()`) at the
        feet; with `gradient=True` `(values, grads)`, `grads` with a trailing axis of length `e`: the tangential gradient
        `J (J^T J)^-1 grad_xi u` in ambient coordinates, `J = dx/dxi` at the foot (a curve: `(du/dxi) x' / |x'|^2`).  The
        values are bitwise those of `gradient=False`; a point without a foot has NaN in every entry."""
        self._open()
        Z, single = _columns(self._name, self._p, self._N, z)
        M, ncomp, e = self.n_points, Z.shape[1], self._e
        out = np.empty((M, ncomp))
        grad = np.empty((M, ncomp, e)) if gradient else None
        if M:
            from .device import _check, _ptr
            Zd = _c_f64(Z)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_closest_evaluate(self._handle, ncomp, _ptr(Zd), _ptr(out), _ptr(grad)))
        vals, g = _shape_values(out, grad, e, single, self._scalar, self._shape)
        return (vals, g) if gradient else vals


def closest_point(geom: Geometry, z, t, max_distance=None, gradient: bool = False, return_element: bool = False,
                  return_distance: bool = False, device_id: int = 0):
    """Evaluate the element-space function `z` on the embedded curve or surface `geom` at the feet of the points `t`:
    a `ClosestPointLocator` built, evaluated and closed; the results are bitwise the locator's.

    Returns the values, followed (in this order) by the tangential gradients with `gradient=True`, the elements with
    `return_element=True` and the distances with `return_distance=True`, as a tuple when more than the values are asked
    for."""
    with ClosestPointLocator(geom, t, max_distance=max_distance, device_id=device_id) as cp:
        res = cp.evaluate(z, gradient=gradient)
        res = list(res) if gradient else [res]
        if return_element:
            res.append(cp.elements)
        if return_distance:
            res.append(cp.distances)
    return res[0] if len(res) == 1 else tuple(res)
