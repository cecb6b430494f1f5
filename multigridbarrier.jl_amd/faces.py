"""The facets of a mesh: `Faces(geom)`, `boundary_flux(geom, z, ...)` and `jump_indicator(geom, z, ...)`.

`Faces` puts a mesh and a Gauss rule on its element faces on the device once (csrc/faces.hip, `mgbhip_faces_*`).  The
device finds which (element, local face) pairs are the two sides of one face and which lie on the boundary, and then
integrates over them: the flux `int |grad u|^(p-2) grad u . n ds` through the boundary or a part of it (capacity, torque,
reaction force, a conservation check against `int f`), and over the interior faces the squared jumps of `u` (the solution
lives in the broken element space, so this measures nonconformity) and of the normal flux, the standard cheap
a-posteriori indicator of where the mesh is too coarse.  The reference has no counterpart.

Families: `fem2d` and `fem3d` Q_k with `1 <= k <= MAX_DEGREE` on flat meshes, `fem2d_P1`, and `fem2d_P2` with 6 or 7
nodes, mapped through all its nodes whatever `curved` says (as `integrate` does).  `fem1d`, embedded curves and
surfaces and the spectral families raise `ValueError`.  Meshes with hanging nodes are not supported: a face whose corner
ids no neighbour shares is taken for a boundary face.

Local faces.  Q_k has `F = 2d` faces, `f = 2a + s` for axis `a` and layer `s` (0: the low side, 1: the high side), the
order of `tensorfem.find_boundary`; the face parameters are the remaining axes in ascending order, lower axis fastest.
A triangle has `F = 3` edges between the corners (0, 1), (1, 2), (2, 0), parametrised by `s` in [-1, 1] from the first
corner to the second.  The rule is Gauss-Legendre with `order = n` points per face axis (`1..10`, default `k + 2`).

The host builds every table (`face_tables`) and checks every argument before any device work; the device sees tables
only.  At point `q` of a face of an element with nodes `x_i` and values `z_i`:

    J = sum_i x_i dphi_i^T,   grad u = J^-T sum_i z_i dphi_i,   n = J^-T n_ref / |J^-T n_ref|,
    ds = wf_q |J t| (2-D) or wf_q |J t1 x J t2| (3-D),   a(grad u) = |grad u|^(p-2) grad u  (0 where grad u = 0).

Results are reproducible bit for bit: a face's value is the sum of its terms in an order fixed by the rule alone, totals
are compensated sums in face or element order, a column does not depend on the columns that ride along and a face does
not depend on the `weight` rows of other faces.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import fem2d_p1, fem2d_p2
from ._handle import DeviceObject
from .fem2d_p1 import FEM2D_P1
from .fem2d_p2 import FEM2D_P2
from .integrate import MAX_ORDER, PLAN_KEYS, gauss_rule_cube, qk_tables, triangle_tables
from .interpolate import MAX_DEGREE, _c_f64
from .multigrid import Geometry
from .spectral import SPECTRAL1D, SPECTRAL2D
from .tensorfem import TensorFEM, _multi_index

KINDS = {"value": 0, "flux": 1}                 # include/mgbhip.h MGBHIP_FACE_*
TRIANGLE_CORNERS = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0]])      # (l1, l2) of the corners, in node order


# ---------------------------------------------------------------------------
# local faces and tables (host, NumPy)
# ---------------------------------------------------------------------------

def _family(geom: Geometry):
    """(name, d, k, p, N, triangle basis table or None, corner slots or None); ValueError if the family has no faces here."""
    disc = geom.discretization
    if isinstance(disc, (SPECTRAL1D, SPECTRAL2D)):
        name = "spectral1d" if isinstance(disc, SPECTRAL1D) else "spectral2d"
        raise ValueError(f"Faces: {name} geometries have one global element and no element faces")
    if isinstance(disc, TensorFEM):
        p, N, e = geom.x.shape
        if disc.d == 1:
            raise ValueError("Faces: fem1d is not supported (the faces of an interval are points)")
        if e != disc.d:
            raise ValueError(f"Faces: embedded meshes are not supported (d = {disc.d} in R^{e}); only flat meshes d = e")
        if disc.d not in (2, 3):
            raise ValueError(f"Faces: TensorFEM with d = {disc.d} is not supported")
        if not 1 <= disc.k <= MAX_DEGREE:
            raise ValueError(f"Faces: element degree k = {disc.k} is outside 1..{MAX_DEGREE}")
        return f"fem{disc.d}d", disc.d, disc.k, p, N, None, None
    if isinstance(disc, FEM2D_P1):
        p, N, _ = geom.x.shape
        return "fem2d_P1", 2, 1, p, N, fem2d_p1.basis_coefficient_table(), (0, 1, 2)
    if isinstance(disc, FEM2D_P2):
        p, N, _ = geom.x.shape
        return "fem2d_P2", 2, 2, p, N, fem2d_p2.basis_coefficient_table(p == 7), (0, 2, 4)
    raise ValueError(f"Faces: no method for {type(disc).__name__} geometries")


def point_permutations(d: int, n: int) -> np.ndarray:
    """`perm (ncode, n^(d-1))`: point `q` of a face seen from its L side is point `perm[code, q]` seen from the R side.

    With `i0`, `i1` the places of L's first two face corners among R's face corners (corner `c` of a face sits at the
    face parameters `(-1)^(1 - bit_j(c))`, lower axis fastest): in 2-D `code = i0` (0: the two parameters run the same
    way, 1: opposite ways); for a quadrilateral face `code = 2 i0 + m`, `m = 0` if L's first face axis runs along R's
    first and 1 if along R's second.  L's parameter -1 on an axis is R's corner bit there, so the axis is reversed
    exactly when that bit of `i0` is set; the Gauss points are symmetric, so reversing an axis is `i -> n - 1 - i`."""
    if d == 2:
        return np.stack([np.arange(n), np.arange(n)[::-1]]).astype(np.int32)
    perm = np.zeros((8, n * n), dtype=np.int32)
    for code in range(8):
        i0, m = code // 2, code % 2
        b0, b1 = i0 & 1, (i0 >> 1) & 1
        for q in range(n * n):
            i, j = q % n, q // n                      # L's indices along its first and second face axis
            if m == 0:
                r0, r1 = (n - 1 - i if b0 else i), (n - 1 - j if b1 else j)
            else:
                r1, r0 = (n - 1 - i if b1 else i), (n - 1 - j if b0 else j)
            perm[code, q] = r0 + n * r1
    return perm


def face_tables(geom: Geometry, order=None) -> dict:
    """What the device is handed for `geom`: `xi (F, Qf, d)`, `wf (Qf,)`, `phi (F, Qf, p)`, `dphi (F, Qf, p, d)`,
    `tangents (F, d-1, d)`, `normals (F, d)`, `corners (F, 2^(d-1))`, `nodes` (per face, every local node on it),
    `perm (ncode, Qf)` and `order`."""
    name, d, k, p, N, table, slots = _family(geom)
    if order is None:
        order = k + 2
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 1 <= int(order) <= MAX_ORDER:
        raise ValueError(f"Faces: order = {order!r} must be an integer in 1..{MAX_ORDER}")
    n = int(order)
    s, wf = gauss_rule_cube(d - 1, n)                                   # face parameters (Qf, d-1), lower axis fastest
    Qf = s.shape[0]
    if table is None:
        F, sn = 2 * d, k + 1
        xi, tangents, normals = np.zeros((F, Qf, d)), np.zeros((F, d - 1, d)), np.zeros((F, d))
        corners, nodes = np.zeros((F, 1 << (d - 1)), dtype=np.int32), []
        for a in range(d):
            rest = [b for b in range(d) if b != a]
            for side in (0, 1):
                f = 2 * a + side
                xi[f, :, a] = 2.0 * side - 1.0
                normals[f, a] = 2.0 * side - 1.0
                for j, b in enumerate(rest):
                    xi[f, :, b] = s[:, j]
                    tangents[f, j, b] = 1.0
                for c in range(1 << (d - 1)):
                    mi = [0] * d
                    mi[a] = side * k
                    for j, b in enumerate(rest):
                        mi[b] = k * ((c >> j) & 1)
                    corners[f, c] = sum(mi[b] * sn ** b for b in range(d))
                nodes.append([lin for lin in range(sn ** d) if _multi_index(lin, sn, d)[a] == side * k])
        tabs = [qk_tables(d, k, xi[f]) for f in range(F)]
    else:
        F = 3
        xi, tangents, normals = np.zeros((F, Qf, 2)), np.zeros((F, 1, 2)), np.zeros((F, 2))
        corners, nodes = np.zeros((F, 2), dtype=np.int32), []
        for f in range(3):
            A, B, Cc = TRIANGLE_CORNERS[f], TRIANGLE_CORNERS[(f + 1) % 3], TRIANGLE_CORNERS[(f + 2) % 3]
            xi[f] = 0.5 * (1.0 - s) * A[None, :] + 0.5 * (1.0 + s) * B[None, :]
            t = 0.5 * (B - A)
            nr = np.array([t[1], -t[0]])
            if nr @ (Cc - A) > 0:
                nr = -nr
            tangents[f, 0], normals[f] = t, nr
            corners[f] = (slots[f], slots[(f + 1) % 3])
            nodes.append([slots[f], slots[(f + 1) % 3]] if p == 3 else [2 * f, 2 * f + 1, (2 * f + 2) % 6])
        tabs = [triangle_tables(table, xi[f]) for f in range(F)]
    phi = np.stack([tb[0] for tb in tabs])
    dphi = np.stack([tb[1] for tb in tabs])
    return dict(xi=xi, wf=wf, phi=phi, dphi=dphi, tangents=tangents, normals=normals, corners=corners, nodes=nodes,
                perm=point_permutations(d, n), order=n)


def plan(d: int, p: int, Qf: int, F: int, sides: int, nfaces: int) -> dict:
    """What `mgbhip_faces_plan` reports for a shape (csrc/faces_layout.hpp `face_decide`, the lane plan of
    csrc/quad_layout.hpp for faces): `sides = 1` the boundary
    kernel, `2` the interior one; needs the library, no device."""
    from .device import _check, load_library
    lib = load_library()
    out = (C.c_int32 * 16)()
    _check(lib, lib.mgbhip_faces_plan(d, p, Qf, F, sides, nfaces, out))
    return dict(zip(PLAN_KEYS, (int(v) for v in out)))


def _iptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _exponent(p) -> float:
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)):
        raise ValueError("Faces: p must be a number")
    p = float(p)
    if not np.isfinite(p) or p < 1.0:
        raise ValueError(f"Faces: p = {p} must be finite and >= 1")
    return p


class _Spec:
    """Everything the host knows before the device is touched: the family, the tables, and the checks of a call."""

    def __init__(self, geom: Geometry, order):
        self.name, self.d, self.k, self.p, self.N, _, _ = _family(geom)
        self.tables = face_tables(geom, order)
        if self.N == 0:
            raise ValueError(f"Faces: the {self.name} geometry has no elements")
        if not np.all(np.isfinite(geom.x)):
            raise ValueError(f"Faces: the {self.name} mesh has non-finite node coordinates")
        t = np.asarray(geom.t)
        if t.shape != (self.p, self.N) or t.min() < 0 or t.max() >= 2 ** 31:
            raise ValueError(f"Faces: geom.t must be ({self.p}, {self.N}) node ids in [0, 2^31)")
        self.order = self.tables["order"]
        self.F, self.Qf = self.tables["xi"].shape[:2]

    def check_call(self, z, kind, p):
        """(Z (p*N, ncol), whether z was a vector, the exponent); ValueError otherwise."""
        if kind not in KINDS:
            raise ValueError(f"Faces: kind must be 'value' or 'flux' (got {kind!r})")
        pexp = _exponent(p)
        Z = np.asarray(z, dtype=np.float64)
        if Z.ndim not in (1, 2):
            raise ValueError(f"Faces: z must be a vector or a matrix (got {Z.ndim} dimensions)")
        single = Z.ndim == 1
        Z = Z.reshape(Z.shape[0], -1)
        if Z.shape[0] != self.p * self.N:
            raise ValueError(f"Faces: a {self.name} function on this mesh has {self.p * self.N} values (z has {Z.shape[0]})")
        if Z.shape[1] < 1:
            raise ValueError("Faces: z has no columns")
        return _c_f64(Z), single, pexp


    def check_weight(self, weight, B=None):
        """`weight` as the device reads it, or None; `B` the number of boundary faces once it is known."""
        if weight is None:
            return None
        W = np.asarray(weight, dtype=np.float64)
        if W.ndim != 2 or W.shape[1] != self.Qf or (B is not None and W.shape[0] != B):
            raise ValueError(f"Faces: weight must be ({'B' if B is None else B}, {self.Qf}), one value per point of points() "
                             f"(got shape {W.shape})")
        return _c_f64(W)


class Faces(DeviceObject):
    """The faces of the mesh of `geom` with a Gauss rule of `order` points per face axis (`1..10`, default `k + 2`),
    resident on the device.  See the module docstring for the families, the local faces and the definitions.

    Topology, fixed by the mesh alone (`geom.t`): `boundary (B, 2)` `[element, face]` in ascending `element * F + face`;
    `interior (I, 4)` `[eL, fL, eR, fR]` in ascending `eL * F + fL`, the lower of the two incidences; `orientation (I,)`
    the code into `perm` (`point_permutations`); `element_faces (N, F)`: an interior face index, or `-1 - b` for boundary
    face `b`.  A face shared by more than two elements and a mesh with `det J <= 0` at a face point are refused
    (`ValueError`).  Hanging nodes are not supported: their unmatched faces appear as boundary faces.

    The object holds copies of what it needs.  Use it as a context manager or call `close()`."""

    _closed_message = "Faces: the faces are closed"
    _destroy = "mgbhip_faces_destroy"

    def __init__(self, geom: Geometry, order=None, device_id: int = 0):
        sp = self._spec = _Spec(geom, order)
        tb = self.tables = sp.tables
        self._d, self._p, self._N, self._F, self._Qf = sp.d, sp.p, sp.N, sp.F, sp.Qf
        self.order, self.n_elements, self.n_local_faces, self.n_points = sp.order, int(sp.N), sp.F, sp.Qf
        self._labels = np.ascontiguousarray(np.asarray(geom.t).T, dtype=np.int64)             # (N, p)
        t32 = np.ascontiguousarray(self._labels, dtype=np.int32)
        from .device import _ptr
        arrs = [_c_f64(geom.xflat), _c_f64(tb["wf"]), _c_f64(tb["phi"]), _c_f64(tb["dphi"]), _c_f64(tb["tangents"]),
                _c_f64(tb["normals"])]
        corners, perm = np.ascontiguousarray(tb["corners"], dtype=np.int32), np.ascontiguousarray(tb["perm"], dtype=np.int32)
        nb, ni = C.c_int64(), C.c_int64()
        self._create(device_id, "mgbhip_faces_create", self._d, self._p, self._N, _ptr(arrs[0]), _iptr(t32), self._F, self._Qf,
                     _ptr(arrs[1]), _ptr(arrs[2]), _ptr(arrs[3]), _ptr(arrs[4]), _ptr(arrs[5]), _iptr(corners), perm.shape[0],
                     _iptr(perm), outputs=(C.byref(nb), C.byref(ni)), invalid_is_value_error=True)
        B, I = int(nb.value), int(ni.value)
        self.n_boundary, self.n_interior = B, I
        self.boundary, self.interior = np.zeros((B, 2), dtype=np.int32), np.zeros((I, 4), dtype=np.int32)
        self.orientation, self.element_faces = np.zeros(I, dtype=np.int32), np.zeros((self._N, self._F), dtype=np.int32)
        from .device import _check
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_topology(self._handle, _iptr(self.boundary), _iptr(self.interior),
                                                                  _iptr(self.orientation), _iptr(self.element_faces)))

    def plan(self, sides: int = 1) -> dict:
        """The launch plan of the boundary (`sides = 1`) or interior (`sides = 2`) kernel of this shape."""
        return plan(self._d, self._p, self._Qf, self._F, sides, self.n_boundary if sides == 1 else self.n_interior)

    def last_times(self) -> dict:
        """Device milliseconds taken with events on the object's stream: `face_ms` the face kernel and `reduce_ms` what
        follows it (the reduction; for `indicator` the gather too) in the last `integrate` / `jumps` / `indicator` call
        (0 before the first), `topology_ms` the topology build."""
        self._open()
        from .device import _check, _ptr
        ms = np.zeros(3)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_times(self._handle, _ptr(ms)))
        return dict(face_ms=float(ms[0]), reduce_ms=float(ms[1]), topology_ms=float(ms[2]))

    def boundary_nodes(self):
        """The `(v, e)` pairs (local node, element) of every node whose global id lies on a boundary face, ascending in
        `e * p + v`: `find_boundary`'s format and, for the Q_k families, its result."""
        self._open()
        isb = np.zeros(int(self._labels.max()) + 1, dtype=bool)
        for f, nodes in enumerate(self.tables["nodes"]):
            els = self.boundary[self.boundary[:, 1] == f, 0]
            isb[self._labels[els][:, nodes].reshape(-1)] = True
        flat = np.nonzero(isb[self._labels.reshape(-1)])[0]
        return [(int(i % self._p), int(i // self._p)) for i in flat]

    def _geometry(self, which: int, points: bool, normals: bool, measures: bool):
        self._open()
        from .device import _check, _ptr
        nf = self.n_boundary if which == 0 else self.n_interior
        P = np.zeros((nf, self._Qf, self._d)) if points else None
        Nn = np.zeros((nf, self._Qf, self._d)) if normals else None
        M = np.zeros((nf, self._Qf)) if measures else None
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_geometry(self._handle, which, _ptr(P), _ptr(Nn), _ptr(M)))
        return P, Nn, M

    def points(self) -> np.ndarray:
        """`(B, Qf, d)`: the physical points of the rule on the boundary faces."""
        return self._geometry(0, True, False, False)[0]

    def normals(self) -> np.ndarray:
        """`(B, Qf, d)`: the unit outward normals at `points()`."""
        return self._geometry(0, False, True, False)[1]

    def measures(self) -> np.ndarray:
        """`(B, Qf)`: `ds`, the measure each boundary point carries; they sum to the measure of the boundary."""
        return self._geometry(0, False, False, True)[2]

    def interior_measures(self) -> np.ndarray:
        """`(I, Qf)`: `ds` on the interior faces, taken from the `L` side."""
        return self._geometry(1, False, False, True)[2]

    def face_sizes(self) -> np.ndarray:
        """`(I,)`: `h_F = |F|^(1/(d-1))`, `|F|` the sum of `interior_measures()` over the face's points in point order."""
        self._open()
        from .device import _check, _ptr
        out = np.zeros(self.n_interior)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_sizes(self._handle, _ptr(out)))
        return out

    def integrate(self, z, kind: str = "flux", p=2.0, weight=None, per_face: bool = False):
        """The integral over the boundary of `u` (`kind="value"`) or of the flux `a(grad u) . n` (`kind="flux"`,
        `a = |grad u|^(p-2) grad u`, `p >= 1`; `p = 2` calls no `pow`, and the flux is 0 where `grad u = 0`), `u` the
        element function with broken-basis values `z` (`(p*N,)`, or `(p*N, ncol)`: one result per column).  `weight`
        `(B, Qf)` multiplies the integrand at `points()`: a selection of faces, or Neumann data.

        Returns a float, or `(ncol,)` for a matrix; with `per_face=True` `(total, values)` with the face values `(B,)` or
        `(B, ncol)`.  The totals are bitwise the same with and without `per_face`."""
        self._open()
        Z, single, pexp = self._spec.check_call(z, kind, p)
        W = self._spec.check_weight(weight, self.n_boundary)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        totals = np.zeros(ncol)
        face = np.zeros((self.n_boundary, ncol)) if per_face else None
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_integrate(self._handle, KINDS[kind], C.c_double(pexp), ncol, _ptr(Z),
                                                                   _ptr(W), _ptr(face), _ptr(totals)))
        total = float(totals[0]) if single else totals
        if not per_face:
            return total
        return total, (face[:, 0].copy() if single else face)

    def jumps(self, z, kind: str = "flux", p=2.0) -> np.ndarray:
        """Per interior face `int (u_L - u_R)^2` (`kind="value"`) or `int (a_L . n_L + a_R . n_R)^2` (`kind="flux"`), each
        side evaluated through its own element map at the matched point; `(I,)` or `(I, ncol)`."""
        self._open()
        Z, single, pexp = self._spec.check_call(z, kind, p)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        out = np.zeros((self.n_interior, ncol))
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_jumps(self._handle, KINDS[kind], C.c_double(pexp), ncol, _ptr(Z), _ptr(out)))
        return out[:, 0].copy() if single else out

    def indicator(self, z, p=2.0):
        """`(eta2, total)`: `eta2_K = sum over the interior faces F of K, in local face order, of (h_F / 2) int_F [flux]^2`
        with `h_F = face_sizes()`, `(N,)` or `(N, ncol)`, gathered through `element_faces` without atomics, and its
        compensated sum over the elements."""
        self._open()
        Z, single, pexp = self._spec.check_call(z, "flux", p)
        from .device import _check, _ptr
        ncol = Z.shape[1]
        eta2, totals = np.zeros((self._N, ncol)), np.zeros(ncol)
        _check(self._ctx.lib, self._ctx.lib.mgbhip_faces_indicator(self._handle, C.c_double(pexp), ncol, _ptr(Z), _ptr(eta2),
                                                                   _ptr(totals)))
        return (eta2[:, 0].copy(), float(totals[0])) if single else (eta2, totals)


def boundary_flux(geom: Geometry, z, p=2.0, weight=None, per_face: bool = False, order=None, device_id: int = 0):
    """`Faces(geom, order).integrate(z, "flux", p, weight, per_face)`: a `Faces` built, called and closed.  Every argument
    that can be checked without the topology is checked before the device is touched."""
    sp = _Spec(geom, order)
    sp.check_call(z, "flux", p)
    sp.check_weight(weight)
    with Faces(geom, order=order, device_id=device_id) as fc:
        return fc.integrate(z, kind="flux", p=p, weight=weight, per_face=per_face)


def jump_indicator(geom: Geometry, z, p=2.0, order=None, device_id: int = 0):
    """`Faces(geom, order).indicator(z, p)`: a `Faces` built, called and closed."""
    _Spec(geom, order).check_call(z, "flux", p)
    with Faces(geom, order=order, device_id=device_id) as fc:
        return fc.indicator(z, p=p)
