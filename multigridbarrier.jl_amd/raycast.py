"""Rays through a solution: `RayCaster` (line integrals and volume rendering along given rays), `camera_rays` and
`render_volume(geom, u, eye, target)`.

The reference's default picture of a `fem3d` solution is a volume render with isosurfaces and optional slices
(ext/MultiGridBarrierPyPlotExt/plot3d.jl:69-149, PyVista on the CPU).  `isocontour()` gives the isosurfaces and the
slices; this module gives the volume render, straight from the elements on the device (csrc/raycast.hip).  Where the
samples of a ray fall, and which element and reference coordinates each sample has, does not depend on the field: a
`RayCaster` is a `PointLocator` whose points are generated on the device, plus a kernel that sums or composites the
values ray by ray.  The host only checks arguments (before any device work), normalises the directions and computes
the clip box.  Nothing here plots or writes image files: the result is a plain array.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from ._handle import DeviceObject
from .interpolate import P1, P2, P2C, QK, _c_f64, _columns, _plan
from .multigrid import Geometry
from .tensorfem import TensorFEM

QK_BOX_PAD = 0.125      # csrc/interp_device.hpp QK_BOX_PAD: a curved Q_k image can leave its nodes' box


def _raycast_plan(geom: Geometry, who: str = "RayCaster", curved_p2: bool = False):
    """`interpolate._plan` restricted to the families rays are cast through; ValueError names the family otherwise.

    Curved fem2d_P2 (`P2C`) is refused by name unless `curved_p2` is set (the field-line tracer sets it): the ray sampler
    clips against the unpadded node box, which a curved domain can leave."""
    disc = geom.discretization
    if isinstance(disc, TensorFEM) and disc.e != disc.d:
        raise ValueError(f"{who}: fem{disc.d}d embedded in {disc.e} dimensions (a manifold) is not supported")
    family, name, d, k, p, N, xnodes, table = _plan(geom)
    if family == P2C and not curved_p2:
        raise ValueError(f"{who}: curved fem2d_P2 geometries are not supported")
    if family not in (QK, P1, P2, P2C):
        raise ValueError(f"{who}: {name} geometries are not supported (fem2d, fem3d, fem2d_P1 and fem2d_P2 are)")
    if N == 0:
        raise ValueError(f"{who}: the {name} geometry has no elements")
    if not np.all(np.isfinite(xnodes)):
        raise ValueError(f"{who}: the {name} mesh has non-finite node coordinates")
    return family, name, d, k, p, N, xnodes, table


def clip_box(geom: Geometry) -> np.ndarray:
    """(2, d): the box rays are clipped against, lo then hi.  The per-axis minimum and maximum of `geom.xflat`; for
    Q_k with k >= 2 every axis is widened by 1/8 of its extent on both sides (a curved image can leave its nodes' box)."""
    family, _, _, k, _, _, xnodes, _ = _raycast_plan(geom, "clip_box")
    lo, hi = xnodes.min(axis=0), xnodes.max(axis=0)
    if family == QK and k >= 2:
        ext = hi - lo
        lo, hi = lo - QK_BOX_PAD * ext, hi + QK_BOX_PAD * ext
    return np.stack([lo, hi])


def _diagonal(box: np.ndarray) -> float:
    ext = box[1] - box[0]
    return float(math.sqrt(float(np.sum(ext * ext))))


def normalize(d: np.ndarray) -> np.ndarray:
    """`d / sqrt(sum d*d)` per row, the squares added in axis order."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):     # the caller refuses what does not normalise
        s = d[:, 0] * d[:, 0]
        for a in range(1, d.shape[1]):
            s = s + d[:, a] * d[:, a]
        return d / np.sqrt(s)[:, None]


def _check_size(size):
    try:
        W, H = size
    except (TypeError, ValueError):
        raise ValueError(f"camera_rays: size must be (W, H) (got {size!r})") from None
    for v in (W, H):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError(f"camera_rays: size entries must be integers >= 1 (got {size!r})")
    return int(W), int(H)


def _vec3(name: str, v) -> np.ndarray:
    a = np.asarray(v, dtype=np.float64)
    if a.shape != (3,) or not np.all(np.isfinite(a)):
        raise ValueError(f"camera_rays: {name} must be three finite numbers (got {v!r})")
    return a


def camera_rays(eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0, height: Optional[float] = None):
    """Origins and directions `(o, d)`, each `(W*H, 3)`, of the rays of a camera at `eye` looking at `target`.

    Ray `r = row * W + col` goes through the centre of pixel `(row, col)`; row 0 is the top row of the image and
    column 0 its left column (seen from the eye with `up` pointing up), so `result.reshape(H, W, ...)` is an image in
    the usual row-major, top-down order.  With `forward = (target - eye) / |target - eye|`, `right = forward x up`
    (normalised) and `upv = right x forward`, pixel `(row, col)` has the image-plane coordinates
    `px = ((col + 0.5) / W - 0.5) * (W / H) * s` and `py = (0.5 - (row + 0.5) / H) * s`.

    - Pinhole (the default): `s = 2 tan(fov / 2)` with the vertical field of view `fov` in degrees, `0 < fov < 180`; all
      origins are `eye` and the directions `forward + px right + py upv` (not normalised: `RayCaster` does that).  The
      top and bottom edges of the image subtend `fov`.
    - Orthographic (`height=...`): `s = height`, the height of the image in world units; all directions are `forward`
      and the origins `eye + px right + py upv`.
    """
    eye, target, up = _vec3("eye", eye), _vec3("target", target), _vec3("up", up)
    W, H = _check_size(size)
    fwd = target - eye
    nf = float(np.linalg.norm(fwd))
    if not nf > 0.0:
        raise ValueError("camera_rays: eye and target coincide")
    fwd = fwd / nf
    right = np.cross(fwd, up)
    nr = float(np.linalg.norm(right))
    if not nr > 1e-12 * float(np.linalg.norm(up)) or not nr > 0.0:
        raise ValueError("camera_rays: up is parallel to the viewing direction (or zero)")
    right = right / nr
    upv = np.cross(right, fwd)
    if height is None:
        if not (isinstance(fov, (int, float, np.integer, np.floating)) and math.isfinite(fov) and 0.0 < fov < 180.0):
            raise ValueError(f"camera_rays: fov must be in (0, 180) degrees (got {fov!r})")
        s = 2.0 * math.tan(math.radians(float(fov)) / 2.0)
    else:
        if not (isinstance(height, (int, float, np.integer, np.floating)) and math.isfinite(height) and height > 0.0):
            raise ValueError(f"camera_rays: height must be finite and positive (got {height!r})")
        s = float(height)
    px = ((np.arange(W) + 0.5) / W - 0.5) * (W / H) * s
    py = (0.5 - (np.arange(H) + 0.5) / H) * s
    off = (py[:, None, None] * upv[None, None, :] + px[None, :, None] * right[None, None, :]).reshape(W * H, 3)
    if height is None:
        return np.broadcast_to(eye, (W * H, 3)).copy(), fwd[None, :] + off
    return eye[None, :] + off, np.broadcast_to(fwd, (W * H, 3)).copy()


def default_transfer(diagonal: float, K: int = 256) -> np.ndarray:
    """The `(K, 4)` table `render` uses when `transfer` is None: colour grows linearly from black to white and the
    extinction sigma linearly from 0 to `4 / diagonal`."""
    ramp = np.arange(K) / (K - 1)
    return np.stack([ramp, ramp, ramp, ramp * (4.0 / diagonal)], axis=1)


def _check_transfer(transfer) -> np.ndarray:
    T = np.asarray(transfer, dtype=np.float64)
    if T.ndim != 2 or T.shape[1] != 4 or T.shape[0] < 2:
        raise ValueError(f"RayCaster.render: transfer must be (K, 4) with K >= 2 (got shape {T.shape})")
    if not np.all(np.isfinite(T)):
        raise ValueError("RayCaster.render: every transfer entry must be finite")
    if np.any(T[:, 3] < 0.0):
        raise ValueError("RayCaster.render: the extinction column sigma must be >= 0")
    return T


def _check_clim(clim, u: np.ndarray):
    if clim is None:
        fin = u[np.isfinite(u)]
        if fin.size == 0:
            raise ValueError("RayCaster.render: u has no finite entry to take the default clim from")
        lo, hi = float(fin.min()), float(fin.max())
        if not lo < hi:
            raise ValueError(f"RayCaster.render: u is constant ({lo}); give clim=(lo, hi)")
        return lo, hi
    try:
        lo, hi = (float(v) for v in clim)
    except (TypeError, ValueError):
        raise ValueError(f"RayCaster.render: clim must be (lo, hi) (got {clim!r})") from None
    if not (math.isfinite(lo) and math.isfinite(hi) and lo < hi):
        raise ValueError(f"RayCaster.render: clim must be finite with lo < hi (got {clim!r})")
    return lo, hi


class RayCaster(DeviceObject):
    """The rays `o + t d` sampled through `geom` once, for integrating or rendering many fields along them.

    `o` and `d` are `(R, dim)` (one ray may be given as `(dim,)`), with `dim` the dimension of the mesh; origins must be
    finite, directions finite and non-zero.  `step` is the wanted distance between samples, `[t_min, t_max]` the part
    of every ray that is used (`t` is arc length; `t_max` may be `inf`).

    Supported: `fem2d` and `fem3d` (Q_k, `1 <= k <= 8`, curved elements included), `fem2d_P1`, `fem2d_P2` (straight
    elements).  `fem1d`, embedded manifolds, the spectral families and curved P2 raise `ValueError`.

    The algorithm (the same on the device and in the NumPy restatement the tests compare it with, tests/raycast_twin.py):

    1. The host normalises each direction, `d / sqrt(sum d*d)`.
    2. The clip box is `clip_box(geom)`.
    3. Slab test per ray from `tmin = t_min`, `tmax = t_max`: for an axis `a` with `d[a] != 0`, `t1 = (lo[a]-o[a])/d[a]`,
       `t2 = (hi[a]-o[a])/d[a]`, `tmin = max(tmin, min(t1, t2))`, `tmax = min(tmax, max(t1, t2))`; an axis with
       `d[a] == 0` misses unless `lo[a] <= o[a] <= hi[a]`.  A ray with `not tmax > tmin` misses: it has no samples.
    4. `n = max(1, floor((tmax - tmin)/step + 0.5))`, `h = (tmax - tmin)/n`; sample `i` is at `t = tmin + (i + 0.5) h`,
       `x[a] = o[a] + t d[a]`: the midpoints of `n` equal steps that tile the ray's chord of the box exactly.  A count
       pass, a scan and an emit pass lay the samples out ray by ray, without atomics.  More than `2**31 - 1` samples
       raise `ValueError`.
    5. The samples are located as `PointLocator` locates points; per sample the element and the reference
       coordinates stay on the device (32 bytes per sample in 3-D, 24 in 2-D), the positions do not.

    Attributes: `nrays`, `nsamples`, `offsets` (`(R+1,)` int64: ray `r` owns samples `offsets[r]:offsets[r+1]`),
    `step_of_ray` (`(R,)`: the step `h` of each ray, 0.0 for a ray without samples) and `length` (`(R,)`: `h` times the
    number of the ray's samples that lie in an element: its length inside the mesh by the midpoint rule).

    Use it as a context manager or call `close()`; a caster of zero rays needs no device and no library.
    """

    _closed_message = "RayCaster: the caster is closed"
    _destroy = "mgbhip_raycast_destroy"

    def __init__(self, geom: Geometry, o, d, step, t_min: float = 0.0, t_max: float = np.inf, device_id: int = 0):
        self._family, self._name, self._d, k, self._p, self._N, xnodes, table = _raycast_plan(geom)
        dim = self._d
        O, D = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
        if O.ndim == 1 and D.ndim == 1:
            O, D = O.reshape(1, -1), D.reshape(1, -1)
        if O.ndim != 2 or O.shape[1] != dim or D.shape != O.shape:
            raise ValueError(f"RayCaster: o and d must both be (R, {dim}) for this {self._name} geometry "
                             f"(got shapes {O.shape} and {D.shape})")
        if not np.all(np.isfinite(O)):
            raise ValueError("RayCaster: every ray origin must be finite")
        if not np.all(np.isfinite(D)):
            raise ValueError("RayCaster: every ray direction must be finite")
        if np.any(np.all(D == 0.0, axis=1)):
            raise ValueError("RayCaster: a ray direction is zero")
        try:
            step, t_min, t_max = float(step), float(t_min), float(t_max)
        except (TypeError, ValueError):
            raise ValueError("RayCaster: step, t_min and t_max must be numbers") from None
        if not (math.isfinite(step) and step > 0.0):
            raise ValueError(f"RayCaster: step must be finite and positive (got {step})")
        if not math.isfinite(t_min):
            raise ValueError(f"RayCaster: t_min must be finite (got {t_min})")
        if not t_max > t_min:
            raise ValueError(f"RayCaster: t_max must be greater than t_min (got t_min = {t_min}, t_max = {t_max})")
        Dn = normalize(D)
        if not np.all(np.abs(np.sum(Dn * Dn, axis=1) - 1.0) <= 1e-12):      # also false for NaN
            raise ValueError("RayCaster: a ray direction is too long or too short to normalise (sum d*d overflows or "
                             "vanishes)")
        self.box = clip_box(geom)
        self.diagonal = _diagonal(self.box)
        self.nrays = R = int(O.shape[0])
        self.nsamples = 0
        self._offsets = self._steps = self._lengths = None
        if R:
            from .device import _ptr
            O, Dn = _c_f64(O), _c_f64(Dn)
            box, xnodes, table = _c_f64(self.box), _c_f64(xnodes), _c_f64(table)
            n = C.c_int64(0)
            self._create(device_id, "mgbhip_raycast_create", self._family, dim, k, self._p, self._N, _ptr(xnodes),
                         _ptr(table), R, _ptr(O), _ptr(Dn), _ptr(box), step, t_min, t_max, outputs=(C.byref(n),),
                         invalid_is_value_error=True)
            self.nsamples = int(n.value)

    @property
    def offsets(self) -> np.ndarray:
        self._open()
        if self._offsets is None:
            off = np.zeros(self.nrays + 1, dtype=np.int64)
            if self.nrays:
                from .device import _check
                _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_offsets(
                    self._handle, off.ctypes.data_as(C.POINTER(C.c_int64))))
            self._offsets = off
        return self._offsets.copy()

    def _fetch_lengths(self):
        if self._steps is None:
            steps, lengths = np.zeros(self.nrays), np.zeros(self.nrays)
            if self.nrays:
                from .device import _check, _ptr
                _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_lengths(self._handle, _ptr(steps), _ptr(lengths)))
            self._steps, self._lengths = steps, lengths

    @property
    def step_of_ray(self) -> np.ndarray:
        self._open()
        self._fetch_lengths()
        return self._steps.copy()

    @property
    def length(self) -> np.ndarray:
        self._open()
        self._fetch_lengths()
        return self._lengths.copy()

    def samples(self) -> np.ndarray:
        """`(S, dim)`: the sample positions, regenerated on the device (they are not kept) and downloaded."""
        self._open()
        pts = np.empty((self.nsamples, self._d))
        if self.nsamples:
            from .device import _check, _ptr
            _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_samples(self._handle, _ptr(pts)))
        return pts

    def integrate(self, z) -> np.ndarray:
        """The midpoint rule of the line integral of the element-space function `z` along every ray: `(R,)` for `z` of
        shape `(p*N,)`, `(R, ncomp)` for `(p*N, ncomp)`, each column bitwise what a 1-column call returns.  Per ray the
        values at its samples are added in sample order, skipping the samples whose value is not finite (outside the
        mesh, or NaN in `z`), and the sum is multiplied by the ray's step."""
        self._open()
        Z, single = _columns(self._name, self._p, self._N, z)
        ncomp = Z.shape[1]
        out = np.zeros((self.nrays, ncomp))
        if self.nrays:
            from .device import _check, _ptr
            Z = _c_f64(Z)
            _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_integrate(self._handle, ncomp, _ptr(Z), _ptr(out)))
        return out[:, 0] if single else out

    def render(self, u, transfer=None, clim=None, layers=None) -> np.ndarray:
        """`(R, 4)` float64: premultiplied colour and alpha of every ray by front-to-back emission-absorption
        compositing of the element-space function `u` (`(p*N,)`).

        `transfer` is `(K, 4)`, `K >= 2`, finite: row `j` holds the colour `r, g, b` and the extinction `sigma >= 0` per
        unit length at the value `lo + j (hi - lo) / (K - 1)`; the default is `default_transfer(self.diagonal)`.  `clim`
        is `(lo, hi)`, finite with `lo < hi`; the default is the minimum and maximum of the finite entries of `u` (a
        constant `u` raises).  Per ray, in sample order from `T = 1, C = 0`, a sample with a finite value `v` does

            s = min(1, max(0, (v - lo)/(hi - lo)));  f = s*(K-1);  j = min(floor(f), K-2);  w = f - j
            row = transfer[j] + w*(transfer[j+1] - transfer[j])
            e = exp(-(sigma*h));  C += (T*(1 - e))*row[:3];  T = T*e

        and a sample whose value is not finite (outside the mesh, or NaN in `u`) contributes nothing.  The result is
        `(C_r, C_g, C_b, 1 - T)`.  There is no early ray termination: every sample is composited.

        `layers=(t_hit, layer)` puts surfaces into the volume (3-D only): `t_hit` is `(R, K)`, `1 <= K <= 8`, ascending
        along every ray with `inf` for a missing entry, and `layer` is `(R, K, 4)`, finite: premultiplied colour and
        alpha, as `TriangleCaster.trace` and `.shade` return them for the same rays.  A layer is applied before sample
        `i` iff `t_hit <= t_i` (`t_i = tmin + (i + 0.5) h`), the finite ones that remain after the last sample, by
        `C += T*layer[:3];  T = T*(1 - layer[3])`; a ray without samples composites its layers alone.  With `None` the
        path without layers runs, unchanged.
        """
        self._open()
        U = np.asarray(u, dtype=np.float64)
        if U.ndim != 1 or U.shape[0] != self._p * self._N:
            raise ValueError(f"RayCaster.render: u must be a vector of {self._p * self._N} values for this "
                             f"{self._name} geometry (got shape {U.shape})")
        T = default_transfer(self.diagonal) if transfer is None else _check_transfer(transfer)
        lo, hi = _check_clim(clim, U)
        if layers is not None:
            try:
                t_hit, layer = layers
            except (TypeError, ValueError):
                raise ValueError("RayCaster.render: layers must be (t_hit, layer)") from None
            TH, LY = np.asarray(t_hit, dtype=np.float64), np.asarray(layer, dtype=np.float64)
            if self._d != 3:
                raise ValueError(f"RayCaster.render: layers need a 3-D mesh (this is a {self._name} geometry)")
            if TH.ndim != 2 or TH.shape[0] != self.nrays or not 1 <= TH.shape[1] <= 8 or LY.shape != TH.shape + (4,):
                raise ValueError(f"RayCaster.render: layers must be ({self.nrays}, K) and ({self.nrays}, K, 4) with K in "
                                 f"1..8 (got shapes {TH.shape} and {LY.shape})")
            if np.any(np.isnan(TH)) or np.any(TH[:, 1:] < TH[:, :-1]):
                raise ValueError("RayCaster.render: the t_hit of layers must ascend along every ray (inf for a missing "
                                 "entry, no NaN)")
            if not np.all(np.isfinite(LY)):
                raise ValueError("RayCaster.render: every entry of the layer of layers must be finite")
        out = np.zeros((self.nrays, 4))
        if self.nrays:
            from .device import _check, _ptr
            U, T = _c_f64(U), _c_f64(T)
            if layers is None:
                _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_render(
                    self._handle, _ptr(U), int(T.shape[0]), _ptr(T), lo, hi, _ptr(out)))
            else:
                TH, LY = _c_f64(TH), _c_f64(LY)
                _check(self._ctx.lib, self._ctx.lib.mgbhip_raycast_render_layers(
                    self._handle, _ptr(U), int(T.shape[0]), _ptr(T), lo, hi, int(TH.shape[1]), _ptr(TH), _ptr(LY),
                    _ptr(out)))
        return out


def render_volume(geom: Geometry, u, eye, target, up=(0, 0, 1), size=(800, 600), fov: float = 30.0,
                  step: Optional[float] = None, transfer=None, clim=None, device_id: int = 0) -> np.ndarray:
    """`(H, W, 4)`: the volume render of the `fem3d` solution `u` seen by the pinhole camera of `camera_rays`; bitwise
    `RayCaster(geom, *camera_rays(eye, target, up, size, fov), step).render(u, transfer, clim).reshape(H, W, 4)`.  The
    default `step` is 1/256 of the diagonal of `clip_box(geom)`.  Row 0 is the top of the image."""
    _, name, d, _, p, N, _, _ = _raycast_plan(geom, "render_volume")
    if d != 3:
        raise ValueError(f"render_volume: {name} geometries are not supported (the camera is 3-D: fem3d only)")
    W, H = _check_size(size)
    o, dirs = camera_rays(eye, target, up, (W, H), fov)
    U = np.asarray(u, dtype=np.float64)
    if U.ndim != 1 or U.shape[0] != p * N:
        raise ValueError(f"render_volume: u must be a vector of {p * N} values for this {name} geometry "
                         f"(got shape {U.shape})")
    if transfer is not None:
        transfer = _check_transfer(transfer)
    clim = _check_clim(clim, U)
    if step is None:
        step = _diagonal(clip_box(geom)) / 256.0
    with RayCaster(geom, o, dirs, step, device_id=device_id) as rc:
        return rc.render(U, transfer, clim).reshape(H, W, 4)
