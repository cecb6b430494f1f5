"""Measuring a solution: `Quadrature(geom)`, `integrate(geom, z, ...)` and `norm(geom, z, ...)`.

`Quadrature` puts a mesh and a quadrature rule on the device once and then integrates element-space functions over the
domain (csrc/quadrature.hip, `mgbhip_quadrature_*`): `int u`, `int |u - g|^p`, `int |grad u - G|^p` and the energy
`int |grad u|^p / p - f u`, per element and in total, for one `z` or for the columns of a matrix (the frames of a
trajectory).  The reference has no counterpart.

The host builds the rule and the element basis at its points and checks every argument before any device work; the
device code sees tables only and knows no element family.  At point `q` of an element with nodes `x_i`:

    x_q = sum_i phi_i(xi_q) x_i,   J = sum_i x_i (grad_xi phi_i(xi_q))^T,   measure_q = w_q sqrt(det J^T J),
    u_q = sum_i phi_i(xi_q) z_i,   grad u = J (J^T J)^-1 sum_i z_i grad_xi phi_i(xi_q),

the tangential gradient on an embedded curve or surface.  fem2d_P2 elements are mapped through all their nodes whatever
`curved` says, exactly as the geometry's own operators are.

Rules.  `rule="gauss"` with `order = n` points per axis (`1 <= n <= 10`, default `k + 2`): tensor Gauss-Legendre on Q_k
elements (exact to degree `2n - 1` per axis), on triangles the conical product of Gauss-Jacobi(1, 0) and Gauss-Legendre
(`n^2` points, exact to total degree `2n - 1`).  `rule="nodal"` puts the points at the element's own nodes, with the
reference weights of the geometry scaled to sum to the reference cell's volume: the result is a true integral for every
family and equals `geom.w @ F / s` with `s = 2` for fem2d_P2 (whose `geom.w` sums to twice the area: the reference
triangle's weights `2 int phi_j` sum to 1 on a triangle of area 1/2) and `s = 1` for every other family.  A nodal rule is
exact to the degree of the element only (Clenshaw-Curtis on Q_k: degree `k`, and `k + 1` for even `k`; degree 1 on
fem2d_P1, 2 on fem2d_P2 and 3 with the bubble).

Results are reproducible bit for bit: an element's value is the sum of its terms in an order fixed by the rule alone, and
the totals are compensated sums over the elements in a fixed order, the same with and without `per_element`, and for a
column the same whichever other columns ride along.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import fem2d_p1, fem2d_p2
from ._handle import DeviceObject
from .fem2d_p1 import FEM2D_P1
from .fem2d_p2 import FEM2D_P2, MONOMIALS
from .interpolate import MAX_DEGREE, _c_f64
from .multigrid import Geometry
from .spectral import SPECTRAL1D, SPECTRAL2D
from .tensorfem import TensorFEM, _multi_index, _tf_nodes, _tf_reference

KINDS = {"value": 0, "lp": 1, "w1p": 2, "energy": 3}        # include/mgbhip.h MGBHIP_QUAD_*
RULES = ("gauss", "nodal")
MAX_ORDER = 10


# ---------------------------------------------------------------------------
# rules and basis tables (host, NumPy)
# ---------------------------------------------------------------------------

def gauss_rule_cube(d: int, n: int):
    """Tensor Gauss-Legendre on [-1, 1]^d: (points (n^d, d), weights (n^d,)), axis 0 fastest; the weights sum to 2^d."""
    from scipy.special import roots_legendre
    t, w = roots_legendre(n)
    pts = np.array([[t[c] for c in _multi_index(q, n, d)] for q in range(n ** d)])
    wts = np.array([np.prod([w[c] for c in _multi_index(q, n, d)]) for q in range(n ** d)])
    return pts, wts


def conical_rule_triangle(n: int):
    """The conical product rule on the reference triangle {l1, l2 >= 0, l1 + l2 <= 1}: Gauss-Jacobi(1, 0) in
    l1 = (1 + t) / 2 and Gauss-Legendre in l2 = (1 - l1)(1 + s) / 2.  (points (n^2, 2), weights (n^2,)); the weights are
    positive, sum to 1/2 and the rule is exact to total degree 2n - 1."""
    from scipy.special import roots_jacobi, roots_legendre
    tj, wj = roots_jacobi(n, 1.0, 0.0)              # weight (1 - t) on [-1, 1]
    tl, wl = roots_legendre(n)
    a = 0.5 * (1.0 + tj)
    b = 0.5 * (1.0 + tl)
    pts = np.array([[a[i], (1.0 - a[i]) * b[j]] for j in range(n) for i in range(n)])
    wts = np.array([wj[i] * wl[j] / 8.0 for j in range(n) for i in range(n)])
    return pts, wts


def lagrange_with_derivative(nodes: np.ndarray, x: float):
    """(L_i(x), L_i'(x)) of the Lagrange basis on `nodes`, as products over the nodes (no cancellation at a node)."""
    s = len(nodes)
    vals, ders = np.zeros(s), np.zeros(s)
    for i in range(s):
        den = np.prod([nodes[i] - nodes[j] for j in range(s) if j != i])
        vals[i] = np.prod([x - nodes[j] for j in range(s) if j != i]) / den
        ders[i] = sum(np.prod([x - nodes[j] for j in range(s) if j != i and j != m]) for m in range(s) if m != i) / den
    return vals, ders


def qk_tables(d: int, k: int, pts: np.ndarray):
    """phi (Q, p) and dphi (Q, p, d) of the Q_k basis (tensor order, axis 0 fastest) at reference points of [-1, 1]^d."""
    nodes = _tf_nodes(k)
    s = k + 1
    Q, p = pts.shape[0], s ** d
    phi, dphi = np.zeros((Q, p)), np.zeros((Q, p, d))
    for q in range(Q):
        ax = [lagrange_with_derivative(nodes, pts[q, a]) for a in range(d)]
        for i in range(p):
            mi = _multi_index(i, s, d)
            phi[q, i] = np.prod([ax[a][0][mi[a]] for a in range(d)])
            for b in range(d):
                dphi[q, i, b] = np.prod([ax[a][1 if a == b else 0][mi[a]] for a in range(d)])
    return phi, dphi


def triangle_tables(table: np.ndarray, pts: np.ndarray):
    """phi (Q, p) and dphi (Q, p, 2) at points (l1, l2) of the reference triangle, from a `basis_coefficient_table`
    (p, 10) over `fem2d_p2.MONOMIALS`."""
    l1, l2 = pts[:, 0], pts[:, 1]
    mono = np.stack([l1 ** i * l2 ** j for (i, j) in MONOMIALS], axis=1)                                        # (Q, 10)
    d1 = np.stack([i * l1 ** max(i - 1, 0) * l2 ** j if i else 0.0 * l1 for (i, j) in MONOMIALS], axis=1)
    d2 = np.stack([j * l1 ** i * l2 ** max(j - 1, 0) if j else 0.0 * l1 for (i, j) in MONOMIALS], axis=1)
    return mono @ table.T, np.stack([d1 @ table.T, d2 @ table.T], axis=2)


def _family(geom: Geometry):
    """(name, d, e, k, p, N, triangle basis table or None) of a geometry; ValueError if there is no quadrature for it."""
    disc = geom.discretization
    if isinstance(disc, (SPECTRAL1D, SPECTRAL2D)):
        name = "spectral1d" if isinstance(disc, SPECTRAL1D) else "spectral2d"
        raise ValueError(f"integrate: no element quadrature for {name} geometries (geom.w is already the exact "
                         "Clenshaw-Curtis rule there: use geom.w @ F)")
    if isinstance(disc, TensorFEM):
        if not (1 <= disc.d <= 3 and disc.d <= disc.e <= 3):
            raise ValueError(f"integrate: TensorFEM with d = {disc.d}, e = {disc.e} is not supported")
        if not 1 <= disc.k <= MAX_DEGREE:
            raise ValueError(f"integrate: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
        p, N, e = geom.x.shape
        return f"fem{disc.d}d", disc.d, e, disc.k, p, N, None
    if isinstance(disc, FEM2D_P1):
        p, N, _ = geom.x.shape
        return "fem2d_P1", 2, 2, 1, p, N, fem2d_p1.basis_coefficient_table()
    if isinstance(disc, FEM2D_P2):
        p, N, _ = geom.x.shape
        return "fem2d_P2", 2, 2, 2, p, N, fem2d_p2.basis_coefficient_table(p == 7)
    raise ValueError(f"integrate: no method for {type(disc).__name__} geometries")


def reference_rule(geom: Geometry, order=None, rule: str = "gauss"):
    """What the device is handed for `geom`: a dict with the reference points `xi` (Q, d), the reference weights `w`
    (Q,), the basis tables `phi` (Q, p) and `dphi` (Q, p, d), and `order` (None for the nodal rule)."""
    name, d, e, k, p, N, table = _family(geom)
    if rule not in RULES:
        raise ValueError(f"integrate: rule must be 'gauss' or 'nodal' (got {rule!r})")
    if rule == "nodal":
        if order is not None:
            raise ValueError("integrate: the nodal rule has the element's own nodes; it takes no order")
        if table is None:
            ref = _tf_reference(d, k)
            xi, w, phi = ref["nodesref"].copy(), ref["wref"].copy(), np.eye(p)
            dphi = np.stack(ref["Daxis"], axis=2)
        elif name == "fem2d_P1":
            xi, w, phi = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]]), np.full(3, 1.0 / 6.0), np.eye(3)
            dphi = triangle_tables(table, xi)[1]
        else:
            R = fem2d_p2.reference_triangle(p == 7)
            xi, w, phi = R["K"][:, :2].copy(), 0.5 * R["w"], np.eye(p)          # half of 2 int phi_j: sums to 1/2
            dphi = np.stack([R["dx"], R["dy"]], axis=2)
        return dict(xi=xi, w=w, phi=phi, dphi=dphi, order=None)
    if order is None:
        order = k + 2
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"integrate: order = {order!r} must be an integer in 1..{MAX_ORDER}")
    order = int(order)
    if table is None:
        xi, w = gauss_rule_cube(d, order)
        phi, dphi = qk_tables(d, k, xi)
    else:
        xi, w = conical_rule_triangle(order)
        phi, dphi = triangle_tables(table, xi)
    return dict(xi=xi, w=w, phi=phi, dphi=dphi, order=order)


# ---------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------

def _columns(name: str, p: int, N: int, z):
    Z = np.asarray(z, dtype=np.float64)
    if Z.ndim not in (1, 2):
        raise ValueError(f"integrate: z must be a vector or a matrix (got {Z.ndim} dimensions)")
    single = Z.ndim == 1
    Z = Z.reshape(Z.shape[0], -1)
    if Z.shape[0] != p * N:
        raise ValueError(f"integrate: a {name} function on this mesh has {p * N} values (z has {Z.shape[0]})")
    if Z.shape[1] < 1:
        raise ValueError("integrate: z has no columns")
    return Z, single


def _exponent(p, allow_inf: bool = False) -> float:
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
        raise ValueError("integrate: p must be a number")
    p = float(p)
    if allow_inf and p == math.inf:
        return p
    if not math.isfinite(p) or p <= 0.0:
        raise ValueError(f"integrate: p = {p} must be finite and > 0" + (" (or inf)" if allow_inf else ""))
    return p


# the slots of mgbhip_quadrature_plan and mgbhip_faces_plan, in order (csrc/quad_layout.hpp `QuadPlan`, then the table bytes)
PLAN_KEYS = ("threads", "S", "G", "chunk", "tables_lds", "reduce_threads", "groups", "grid", "lds", "table_bytes")


def plan(d: int, e: int, p: int, Q: int, N: int) -> dict:
    """What `mgbhip_quadrature_plan` reports for a shape (csrc/quad_layout.hpp `quad_decide`); needs the library, no device."""
    from .device import _check, load_library
    lib = load_library()
    out = (C.c_int32 * 16)()
    _check(lib, lib.mgbhip_quadrature_plan(d, e, p, Q, N, out))
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


class _Spec:
    """Everything the host knows before the device is touched: the family, the rule with its tables, and the checks of
    a call's arguments."""

    def __init__(self, geom: Geometry, order, rule):
        self.name, self.d, self.e, self.k, self.p, self.N, _ = _family(geom)
        ref = reference_rule(geom, order, rule)
        if self.N == 0:
            raise ValueError(f"integrate: the {self.name} geometry has no elements")
        if not np.all(np.isfinite(geom.x)):
            raise ValueError(f"integrate: the {self.name} mesh has non-finite node coordinates")
        self.rule, self.order = rule, ref["order"]
        self.xi, self.wref, self.phi, self.dphi = ref["xi"], ref["w"], ref["phi"], ref["dphi"]
        self.Q = int(self.xi.shape[0])

    def minus(self, kind: str, minus, ncol: int):
        """`minus` broadcast to what the device reads: (N, Q, ncol) for lp, (N, Q, ncol, e) for w1p; None stays None."""
        if minus is None:
            return None
        if kind not in ("lp", "w1p"):
            raise ValueError(f"integrate: minus goes with kind='lp' or kind='w1p' (got kind={kind!r})")
        M = np.asarray(minus, dtype=np.float64)
        N, Q, e = self.N, self.Q, self.e
        if kind == "lp":
            if M.shape == (N, Q):
                M = M[:, :, None]
            if M.shape not in ((N, Q, 1), (N, Q, ncol)):
                raise ValueError(f"integrate: minus must hold g at points() as ({N}, {Q}) or ({N}, {Q}, {ncol}) "
                                 f"(got shape {np.shape(minus)})")
            return _c_f64(np.broadcast_to(M, (N, Q, ncol)))
        if M.shape != (N, Q, e):
            raise ValueError(f"integrate: minus must hold G at points() as ({N}, {Q}, {e}) (got shape {np.shape(minus)})")
        return _c_f64(np.broadcast_to(M[:, :, None, :], (N, Q, ncol, e)))

    def check_call(self, z, kind, minus, source):
        """(Z (p*N, ncol), whether z was a vector, minus for the device or None, source or None); ValueError otherwise."""
        if kind not in KINDS:
            raise ValueError(f"integrate: kind must be one of {', '.join(repr(k) for k in KINDS)} (got {kind!r})")
        Z, single = _columns(self.name, self.p, self.N, z)
        M = self.minus(kind, minus, Z.shape[1])
        F = None
        if kind == "energy":
            if source is None:
                raise ValueError("integrate: kind='energy' needs source=f, an element-space field")
            F = np.asarray(source, dtype=np.float64)
            if F.shape != (self.p * self.N,):
                raise ValueError(f"integrate: source must be a vector of {self.p * self.N} values (got shape {F.shape})")
            F = _c_f64(F)
        elif source is not None:
            raise ValueError(f"integrate: source goes with kind='energy' (got kind={kind!r})")
        return _c_f64(Z), single, M, F


def _norm_exponent(kind, p) -> float:
    if kind not in ("lp", "w1p"):
        raise ValueError(f"integrate: norm takes kind='lp' or kind='w1p' (got {kind!r})")
    return _exponent(p, allow_inf=True)


class Quadrature(DeviceObject):
    """A quadrature rule on the mesh of `geom`, resident on the device: `rule="gauss"` with `order` points per axis
    (`1..10`, default `k + 2`) or `rule="nodal"` (see the module docstring for both, and for the factor between the
    nodal rule and `geom.w`).

    Supported: `fem1d`, `fem2d`, `fem3d` with `1 <= k <= 8`, flat or embedded (`fem1d` in R^2 / R^3, `fem2d` in R^3),
    `fem2d_P1`, and `fem2d_P2` with or without the bubble; `spectral1d` / `spectral2d` raise `ValueError`.  The object
    holds copies of what it needs.  Use it as a context manager or call `close()`.

    `n_elements` N, `n_points` Q (per element), `xi` (Q, d) and `wref` (Q,) the rule on the reference cell, `phi` (Q, p)
    and `dphi` (Q, p, d) the basis at its points."""

    _closed_message = "Quadrature: the quadrature is closed"
    _destroy = "mgbhip_quadrature_destroy"

    def __init__(self, geom: Geometry, order=None, rule: str = "gauss", device_id: int = 0):
        sp = self._spec = _Spec(geom, order, rule)
        self._d, self._e, self._p, self._N = sp.d, sp.e, sp.p, sp.N
        self.rule, self.order = sp.rule, sp.order
        self.xi, self.wref, self.phi, self.dphi = sp.xi, sp.wref, sp.phi, sp.dphi
        self.n_elements, self.n_points = int(sp.N), sp.Q
        from .device import _ptr
        x, w, phi, dphi = _c_f64(geom.xflat), _c_f64(self.wref), _c_f64(self.phi), _c_f64(self.dphi)
        self._create(device_id, "mgbhip_quadrature_create", self._d, self._e, self._p, self._N, _ptr(x), self.n_points,
                     _ptr(w), _ptr(phi), _ptr(dphi))

    def plan(self) -> dict:
        """The launch plan of this shape: `plan(d, e, p, Q, N)`."""
        return plan(self._d, self._e, self._p, self.n_points, self._N)

    def last_times(self) -> dict:
        """Device milliseconds of the last `integrate` / `norm` call, taken with events on the object's stream:
        `element_ms` the element kernel, `reduce_ms` the reduction over the elements."""
        self._open()
        from .device import _check, _ptr
        ms = np.zeros(2)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_quadrature_times(self._handle, _ptr(ms)))
        return dict(element_ms=float(ms[0]), reduce_ms=float(ms[1]))

    def points(self) -> np.ndarray:
        """`(N, Q, e)`: the physical quadrature points `x_q = sum_i phi_i(xi_q) x_i`."""
        self._open()
        from .device import _check, _ptr
        out = np.empty((self._N, self.n_points, self._e))
        _check(self._ctx.lib, self._ctx.lib.mgbhip_quadrature_points(self._handle, _ptr(out)))
        return out

    def weights(self) -> np.ndarray:
        """`(N, Q)`: `w_q sqrt(det J^T J)`, the measure each point carries; they sum to the measure of the mesh."""
        self._open()
        from .device import _check, _ptr
        out = np.empty((self._N, self.n_points))
        _check(self._ctx.lib, self._ctx.lib.mgbhip_quadrature_weights(self._handle, _ptr(out)))
        return out

    def _check_call(self, z, kind, minus, source):
        self._open()
        return self._spec.check_call(z, kind, minus, source)

    def integrate(self, z, kind: str = "value", p=2.0, minus=None, source=None, per_element: bool = False):
        """The integral over the mesh of `F(u)`, `u` the element function with broken-basis values `z` (`(p*N,)`, or
        `(p*N, ncol)`: one result per column):

        - `kind="value"`: `u`;  `kind="lp"`: `|u - g|^p`;  `kind="w1p"`: `|grad u - G|^p` (Euclidean norm in R^e; the
          tangential gradient on an embedded manifold);  `kind="energy"`: `|grad u|^p / p - f u` with `source=f`, an
          element-space field `(p*N,)` carried to the points by the same basis.
        - `minus` is `g` as `(N, Q)` or `(N, Q, ncol)`, or `G` as `(N, Q, e)`, at `points()`: evaluate the exact solution
          there, and an error norm carries no interpolation error.
        - `p` is finite and `> 0`; `p = 1` and `p = 2` call no `pow`, and `"w1p"` at `p = 2` takes no square root.

        Returns a float, or `(ncol,)` for a matrix; with `per_element=True` `(total, values)` with the element values
        `(N,)` or `(N, ncol)`.  The totals are bitwise the same with and without `per_element`."""
        Z, single, M, F = self._check_call(z, kind, minus, source)
        pexp = _exponent(p)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        totals = np.empty(ncol)
        elem = np.empty((self._N, ncol)) if per_element else None
        _check(self._ctx.lib, self._ctx.lib.mgbhip_quadrature_integrate(
            self._handle, KINDS[kind], C.c_double(pexp), ncol, _ptr(Z), _ptr(M), _ptr(F), _ptr(elem), _ptr(totals)))
        total = float(totals[0]) if single else totals
        if not per_element:
            return total
        return total, (elem[:, 0].copy() if single else elem)

    def norm(self, z, p=2.0, kind: str = "lp", minus=None):
        """`integrate(z, kind, p, minus) ** (1 / p)` for `kind="lp"` (the L^p norm of `u - g`) or `kind="w1p"` (the
        W^{1,p} seminorm of `u - G`'s potential); `p = inf` is the largest `|u_q - g_q|` resp. `|grad u - G|` over the
        quadrature points, found by a max reduction and therefore exact."""
        self._open()
        pexp = _norm_exponent(kind, p)
        if pexp != math.inf:
            r = self.integrate(z, kind=kind, p=pexp, minus=minus)
            return r ** (1.0 / pexp)
        Z, single, M, _ = self._check_call(z, kind, minus, None)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        out = np.empty(ncol)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_quadrature_max(self._handle, KINDS[kind], ncol, _ptr(Z), _ptr(M), _ptr(out)))
        return float(out[0]) if single else out


def integrate(geom: Geometry, z, kind: str = "value", p=2.0, minus=None, source=None, per_element: bool = False,
              order=None, rule: str = "gauss", device_id: int = 0):
    """`Quadrature(geom, order, rule).integrate(z, ...)`: a `Quadrature` built, called and closed; the results are bitwise
    the object's.  Every argument is checked before the device is touched."""
    _Spec(geom, order, rule).check_call(z, kind, minus, source)
    _exponent(p)
    with Quadrature(geom, order=order, rule=rule, device_id=device_id) as q:
        return q.integrate(z, kind=kind, p=p, minus=minus, source=source, per_element=per_element)


def norm(geom: Geometry, z, p=2.0, kind: str = "lp", minus=None, order=None, rule: str = "gauss", device_id: int = 0):
    """`Quadrature(geom, order, rule).norm(z, ...)`: a `Quadrature` built, called and closed."""
    _norm_exponent(kind, p)
    _Spec(geom, order, rule).check_call(z, kind, minus, None)
    with Quadrature(geom, order=order, rule=rule, device_id=device_id) as q:
        return q.norm(z, p=p, kind=kind, minus=minus)
