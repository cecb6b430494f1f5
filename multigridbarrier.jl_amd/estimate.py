"""The residual a-posteriori estimator: `ResidualEstimator(geom)`, `residual_estimator(geom, z, source, ...)` and
`strong_residual(geom, z, source, ...)`.

`Faces.indicator` measures the flux jumps over the interior faces, `sum_F h_F / 2 int_F [a(grad u) . n]^2`.  This module
adds the other half of the standard residual estimator of the p-Laplace problems the package solves, the
element-interior residual `h_K^2 int_K (f + div a(grad u))^2` (csrc/residual.hip, `mgbhip_residual_*`), and the object
that adds the two.  The reference has no counterpart.

The sign convention is that of `integrate(kind="energy")`, `int |grad u|^p / p - f u`, whose Euler-Lagrange equation is
`-div a(grad u) = f` with `a(g) = |g|^(p-2) g`.  Flat meshes only.  At point `q` of an element with nodes `x_i` and values
`z_i`, with the `J` and `grad u` of `integrate.py`:

    H_xi(v)[b][c] = sum_i v_i d2phi_i / dxi_b dxi_c           (v = z, and v = each coordinate x_a of the nodes)
    H = J^-T ( H_xi(z) - sum_a (grad u)_a H_xi(x_a) ) J^-1    the physical Hessian of u; exact on curved elements too
    div a = |g|^(p-2) ( tr H + (p - 2) g^T H g / |g|^2 ),  g = grad u      (p = 2: tr H;  g = 0 and p != 2: 0)
    r_q = f_q + div a                                         the strong residual
    |K| = sum_q w_q det J  (in point order),   h_K = |K|^(1/d)
    interior_K = h_K^2 sum_q w_q det J r_q^2,      eta2_K = interior_K + Faces.indicator(z, p)[K]

The host builds the rule (`integrate.reference_rule(geom, order, "gauss")`, default order `k + 2`) and the tables,
`d2phi (Q, p, d(d+1)/2)` among them, and checks every argument before any device work; the device sees tables only.
Families: those of `Faces`.  `source` is `f` as an element-space field `(p*N,)`, carried to the points by `phi` as the
energy's source is, or as values at `points()`, `(N, Q)`: the exact `f` then has no interpolation error.

Results are reproducible bit for bit, with the guarantees of `integrate`.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._handle import DeviceObject
from .faces import Faces
from .faces import _Spec as _FaceSpec
from .fem2d_p1 import FEM2D_P1
from .fem2d_p2 import FEM2D_P2, MONOMIALS
from .integrate import PLAN_KEYS, reference_rule
from .integrate import _family as _quad_family
from .interpolate import MAX_DEGREE, _c_f64
from .multigrid import Geometry
from .spectral import SPECTRAL1D, SPECTRAL2D
from .tensorfem import TensorFEM, _multi_index, _tf_nodes


# ---------------------------------------------------------------------------
# second-derivative tables (host, NumPy)
# ---------------------------------------------------------------------------

def second_index_pairs(d: int):
    """The index pairs (b, c), b <= c, in the order of the tables: (0,0), (0,1), (1,1) for d = 2 and (0,0), (0,1),
    (0,2), (1,1), (1,2), (2,2) for d = 3."""
    return [(b, c) for b in range(d) for c in range(b, d)]


def lagrange_with_two_derivatives(nodes: np.ndarray, x: float):
    """(L_i(x), L_i'(x), L_i''(x)) of the Lagrange basis on `nodes`, as products over the nodes (no cancellation at a
    node), like `integrate.lagrange_with_derivative`."""
    s = len(nodes)
    vals, d1, d2 = np.zeros(s), np.zeros(s), np.zeros(s)
    for i in range(s):
        rest = [j for j in range(s) if j != i]
        den = np.prod([nodes[i] - nodes[j] for j in rest])
        vals[i] = np.prod([x - nodes[j] for j in rest]) / den
        d1[i] = sum(np.prod([x - nodes[j] for j in rest if j != m]) for m in rest) / den
        d2[i] = sum(np.prod([x - nodes[j] for j in rest if j != m and j != n]) for m in rest for n in rest if n != m) / den
    return vals, d1, d2


def qk_second_tables(d: int, k: int, pts: np.ndarray) -> np.ndarray:
    """d2phi (Q, p, d(d+1)/2) of the Q_k basis (tensor order, axis 0 fastest) at reference points of [-1, 1]^d: per axis
    `L''` where both derivatives fall on it, `L'` where one does, `L` elsewhere."""
    nodes = _tf_nodes(k)
    s = k + 1
    Q, p = pts.shape[0], s ** d
    pairs = second_index_pairs(d)
    out = np.zeros((Q, p, len(pairs)))
    for q in range(Q):
        ax = [lagrange_with_two_derivatives(nodes, pts[q, a]) for a in range(d)]
        for i in range(p):
            mi = _multi_index(i, s, d)
            for m, (b, c) in enumerate(pairs):
                out[q, i, m] = np.prod([ax[a][(a == b) + (a == c)][mi[a]] for a in range(d)])
    return out


def triangle_second_tables(table: np.ndarray, pts: np.ndarray) -> np.ndarray:
    """d2phi (Q, p, 3) at points (l1, l2) of the reference triangle, from a `basis_coefficient_table` (p, 10) over
    `fem2d_p2.MONOMIALS`: the monomials differentiated twice.  A table of degree 1 gives exact zeros."""
    l1, l2 = pts[:, 0], pts[:, 1]
    zero = 0.0 * l1
    d11 = np.stack([i * (i - 1) * l1 ** max(i - 2, 0) * l2 ** j if i >= 2 else zero for (i, j) in MONOMIALS], axis=1)
    d12 = np.stack([i * j * l1 ** max(i - 1, 0) * l2 ** max(j - 1, 0) if i and j else zero for (i, j) in MONOMIALS], axis=1)
    d22 = np.stack([j * (j - 1) * l1 ** i * l2 ** max(j - 2, 0) if j >= 2 else zero for (i, j) in MONOMIALS], axis=1)
    return np.stack([d11 @ table.T, d12 @ table.T, d22 @ table.T], axis=2)


def _family(geom: Geometry):
    """(name, d, k, p, N, triangle basis table or None); ValueError if the family has no element residual here."""
    disc = geom.discretization
    if isinstance(disc, (SPECTRAL1D, SPECTRAL2D)):
        name = "spectral1d" if isinstance(disc, SPECTRAL1D) else "spectral2d"
        raise ValueError(f"ResidualEstimator: {name} geometries have one global element and no element faces")
    if isinstance(disc, TensorFEM):
        p, N, e = geom.x.shape
        if disc.d == 1:
            raise ValueError("ResidualEstimator: fem1d is not supported (the faces of an interval are points)")
        if e != disc.d:
            raise ValueError(f"ResidualEstimator: embedded meshes are not supported (d = {disc.d} in R^{e}); only flat "
                             "meshes d = e")
        if disc.d not in (2, 3):
            raise ValueError(f"ResidualEstimator: TensorFEM with d = {disc.d} is not supported")
        if not 1 <= disc.k <= MAX_DEGREE:
            raise ValueError(f"ResidualEstimator: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
        return f"fem{disc.d}d", disc.d, disc.k, p, N, None
    if isinstance(disc, (FEM2D_P1, FEM2D_P2)):
        name, d, _, k, p, N, table = _quad_family(geom)
        return name, d, k, p, N, table
    raise ValueError(f"ResidualEstimator: no method for {type(disc).__name__} geometries")


def residual_tables(geom: Geometry, order=None) -> dict:
    """What the device is handed for `geom`: the dict of `integrate.reference_rule(geom, order, "gauss")` (`xi`, `w`,
    `phi`, `dphi`, `order`) with `d2phi (Q, p, d(d+1)/2)` added."""
    name, d, k, p, N, table = _family(geom)
    try:
        ref = dict(reference_rule(geom, order, "gauss"))
    except ValueError as err:
        raise ValueError(str(err).replace("integrate:", "ResidualEstimator:", 1)) from None
    ref["d2phi"] = qk_second_tables(d, k, ref["xi"]) if table is None else triangle_second_tables(table, ref["xi"])
    return ref


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------

def _exponent(p) -> float:
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
        raise ValueError("ResidualEstimator: p must be a number")
    p = float(p)
    if not math.isfinite(p) or p < 1.0:
        raise ValueError(f"ResidualEstimator: p = {p} must be finite and >= 1")
    return p


def plan(d: int, p: int, Q: int, N: int) -> dict:
    """What `mgbhip_residual_plan` reports for a shape (csrc/residual.hpp `residual_decide`, the lane plan of
    csrc/quad_layout.hpp with the longer tables); needs the library, no device."""
    from .device import _check, load_library
    lib = load_library()
    out = (C.c_int32 * 16)()
    _check(lib, lib.mgbhip_residual_plan(d, p, Q, N, out))
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


class _Spec:
    """Everything the host knows before the device is touched: the family, the rule with its tables, and the checks of
    a call's arguments."""

    def __init__(self, geom: Geometry, order):
        self.name, self.d, self.k, self.p, self.N, _ = _family(geom)
        self.tables = residual_tables(geom, order)
        if self.N == 0:
            raise ValueError(f"ResidualEstimator: the {self.name} geometry has no elements")
        if not np.all(np.isfinite(geom.x)):
            raise ValueError(f"ResidualEstimator: the {self.name} mesh has non-finite node coordinates")
        self.order = self.tables["order"]
        self.Q = int(self.tables["xi"].shape[0])

    def check_call(self, z, source, p):
        """(Z (p*N, ncol), whether z was a vector, the source for the device, whether it holds values at the points, the
        exponent); ValueError otherwise."""
        pexp = _exponent(p)
        Z = np.asarray(z, dtype=np.float64)
        if Z.ndim not in (1, 2):
            raise ValueError(f"ResidualEstimator: z must be a vector or a matrix (got {Z.ndim} dimensions)")
        single = Z.ndim == 1
        Z = Z.reshape(Z.shape[0], -1)
        if Z.shape[0] != self.p * self.N:
            raise ValueError(f"ResidualEstimator: a {self.name} function on this mesh has {self.p * self.N} values "
                             f"(z has {Z.shape[0]})")
        if Z.shape[1] < 1:
            raise ValueError("ResidualEstimator: z has no columns")
        if source is None:
            raise ValueError("ResidualEstimator: source=f is needed, an element-space field or values at points()")
        F = np.asarray(source, dtype=np.float64)
        if F.ndim == 1:
            if F.shape != (self.p * self.N,):
                raise ValueError(f"ResidualEstimator: an element-space source is a vector of {self.p * self.N} values "
                                 f"(got shape {F.shape})")
        elif F.ndim == 2:
            if F.shape != (self.N, self.Q):
                raise ValueError(f"ResidualEstimator: a source at points() is ({self.N}, {self.Q}) (got shape {F.shape})")
        else:
            raise ValueError(f"ResidualEstimator: source must be a vector ({self.p * self.N},) or values at points() "
                             f"({self.N}, {self.Q}) (got {F.ndim} dimensions)")
        return _c_f64(Z), single, _c_f64(F), F.ndim == 2, pexp


class ResidualEstimator(DeviceObject):
    """The residual estimator on the mesh of `geom`, resident on the device: a Gauss rule of `order` points per axis
    (`1..10`, default `k + 2`) with the second derivatives of the basis for the element residual, and a
    `Faces(geom, face_order)` for the jumps (attribute `faces`).  See the module docstring for the definitions.

    Supported: the families of `Faces` (`fem2d` / `fem3d` Q_k with `1 <= k <= 8` on flat meshes, `fem2d_P1`, `fem2d_P2`
    with or without the bubble, mapped through all its nodes); `fem1d`, embedded meshes and the spectral families raise
    `ValueError`, and so does a mesh with `det J <= 0` at a point of the rule.  The object holds copies of what it needs.
    Use it as a context manager or call `close()`.

    `n_elements` N, `n_points` Q (per element), `xi`, `wref`, `phi`, `dphi` as on `Quadrature`, and `d2phi`
    `(Q, p, d(d+1)/2)`."""

    _closed_message = "ResidualEstimator: the estimator is closed"
    _destroy = "mgbhip_residual_destroy"
    faces = None

    def __init__(self, geom: Geometry, order=None, face_order=None, device_id: int = 0):
        sp = self._spec = _Spec(geom, order)
        _FaceSpec(geom, face_order)                       # the checks of Faces, before any device work
        tb = sp.tables
        self._d, self._p, self._N = sp.d, sp.p, sp.N
        self.order, self.n_elements, self.n_points = sp.order, int(sp.N), sp.Q
        self.xi, self.wref, self.phi, self.dphi, self.d2phi = tb["xi"], tb["w"], tb["phi"], tb["dphi"], tb["d2phi"]
        from .device import _ptr
        arrs = [_c_f64(geom.xflat), _c_f64(self.wref), _c_f64(self.phi), _c_f64(self.dphi), _c_f64(self.d2phi)]
        self._create(device_id, "mgbhip_residual_create", self._d, self._p, self._N, _ptr(arrs[0]), self.n_points,
                     _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]), _ptr(arrs[4]), invalid_is_value_error=True)
        try:
            self.faces = Faces(geom, order=face_order, device_id=device_id)
        except Exception:
            self.close()
            raise

    def close(self):
        """Free the device state of the estimator and of its `Faces`; calling it again does nothing."""
        if self.faces is not None:
            self.faces.close()
        super().close()

    def plan(self) -> dict:
        """The launch plan of the element-residual kernel of this shape: `plan(d, p, Q, N)`."""
        return plan(self._d, self._p, self.n_points, self._N)

    def last_times(self) -> dict:
        """Device milliseconds of the last `strong_residual` / `interior` / `estimate` call on the element residual, taken
        with events on the object's stream: `element_ms` the element kernel, `reduce_ms` the reduction over the elements
        (0 after `strong_residual`).  The jumps' times are `faces.last_times()`."""
        self._open()
        from .device import _check, _ptr
        ms = np.zeros(2)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_residual_times(self._handle, _ptr(ms)))
        return dict(element_ms=float(ms[0]), reduce_ms=float(ms[1]))

    def _geometry(self, points: bool, weights: bool, sizes: bool):
        self._open()
        from .device import _check, _ptr
        P = np.empty((self._N, self.n_points, self._d)) if points else None
        W = np.empty((self._N, self.n_points)) if weights else None
        H = np.empty(self._N) if sizes else None
        _check(self._ctx.lib, self._ctx.lib.mgbhip_residual_geometry(self._handle, _ptr(P), _ptr(W), _ptr(H)))
        return P, W, H

    def points(self) -> np.ndarray:
        """`(N, Q, d)`: the physical quadrature points `x_q = sum_i phi_i(xi_q) x_i`."""
        return self._geometry(True, False, False)[0]

    def weights(self) -> np.ndarray:
        """`(N, Q)`: `w_q det J`, the measure each point carries; they sum to the measure of the mesh."""
        return self._geometry(False, True, False)[1]

    def element_sizes(self) -> np.ndarray:
        """`(N,)`: `h_K = |K|^(1/d)`, `|K|` the sum of `weights()` over the element's points in point order."""
        return self._geometry(False, False, True)[2]

    def strong_residual(self, z, source, p=2.0) -> np.ndarray:
        """`r = f + div a(grad u)` at `points()`, `(N, Q)`, or `(N, Q, ncol)` for a matrix `z`: what a manufactured
        solution is checked with.  `p = 2` calls no `pow`."""
        self._open()
        Z, single, F, at_points, pexp = self._spec.check_call(z, source, p)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        r = np.empty((self._N, self.n_points, ncol))
        _check(self._ctx.lib, self._ctx.lib.mgbhip_residual_pointwise(self._handle, C.c_double(pexp), ncol, _ptr(Z), _ptr(F),
                                                                      int(at_points), _ptr(r)))
        return r[:, :, 0].copy() if single else r

    def interior(self, z, source, p=2.0):
        """`(values, total)`: `interior_K = h_K^2 int_K r^2` per element, `(N,)` or `(N, ncol)`, and its sum over the
        elements, compensated on the device."""
        self._open()
        Z, single, F, at_points, pexp = self._spec.check_call(z, source, p)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        vals, totals = np.empty((self._N, ncol)), np.empty(ncol)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_residual_integrate(self._handle, C.c_double(pexp), ncol, _ptr(Z), _ptr(F),
                                                                      int(at_points), _ptr(vals), _ptr(totals)))
        return (vals[:, 0].copy(), float(totals[0])) if single else (vals, totals)

    def estimate(self, z, source, p=2.0):
        """`(eta2, total)`: `eta2_K = interior_K + faces.indicator(z, p)[K]`, added per element on the host (one rounding
        each), `(N,)` or `(N, ncol)`, and `math.fsum` of each column: exactly rounded and free of any order."""
        self._open()
        self._spec.check_call(z, source, p)
        inner, _ = self.interior(z, source, p)
        jump, _ = self.faces.indicator(z, p)
        eta2 = inner + jump
        if eta2.ndim == 1:
            return eta2, math.fsum(eta2)
        return eta2, np.array([math.fsum(eta2[:, c]) for c in range(eta2.shape[1])])


def residual_estimator(geom: Geometry, z, source, p=2.0, order=None, face_order=None, device_id: int = 0):
    """`ResidualEstimator(geom, order, face_order).estimate(z, source, p)`: an estimator built, called and closed; the
    results are bitwise the object's.  Every argument is checked before the device is touched."""
    _Spec(geom, order).check_call(z, source, p)
    _FaceSpec(geom, face_order)
    with ResidualEstimator(geom, order=order, face_order=face_order, device_id=device_id) as est:
        return est.estimate(z, source, p=p)


def strong_residual(geom: Geometry, z, source, p=2.0, order=None, device_id: int = 0):
    """`ResidualEstimator(geom, order).strong_residual(z, source, p)`: an estimator built, called and closed."""
    _Spec(geom, order).check_call(z, source, p)
    with ResidualEstimator(geom, order=order, device_id=device_id) as est:
        return est.strong_residual(z, source, p=p)
