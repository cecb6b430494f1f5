"""Field lines of a solution: `StreamTracer` (the mesh, its location grid and one field resident on the device, many
traces) and `streamlines(geom, z, seeds, ...)`.

`interpolate`, `PointLocator`, `isocontour` and the ray casters evaluate a field at points that are known before the
kernel starts.  Following a field is different: every point depends on the value at the previous one.  On the host that
costs one `interpolate()` round trip per Runge-Kutta stage; here one lane of a kernel (csrc/stream.hip) stays on one line
and locates and evaluates again at every stage, with the device functions of `interpolate()` itself, so a stage velocity
is bitwise what `interpolate()` returns at that point.  The velocity of `Zoo.norton_hoff`, the vector solutions of
`Zoo.p_harmonic` (`field="vector"`), the flux lines of the p-Laplacian and the steepest-descent lines of
`minimal_surface` or `elastoplastic_torsion` (`field="gradient"`, `direction="backward"` for descent) are traced this
way.  The host only checks arguments (before any device work) and joins the two halves of `direction="both"`.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._handle import DeviceObject
from .interpolate import _c_f64
from .multigrid import Geometry
from .raycast import _raycast_plan

# include/mgbhip.h MGBHIP_STREAM_*: how a line ended
MAX_STEPS, LEFT, STALLED, OUTSIDE = range(4)
# include/mgbhip.h MGBHIP_STREAM_VECTOR / MGBHIP_STREAM_GRADIENT
_FIELDS = {"vector": 0, "gradient": 1}
_DIRECTIONS = ("forward", "backward", "both")


class Streamlines:
    """The lines of one trace.

    - `points`: `(S, max_steps + 1, d)` float64, the points of each line (row 0 is the seed), NaN beyond each line's end;
      `(S, 2*max_steps + 1, d)` for `direction="both"`.
    - `n`: `(S,)` int32, the number of valid points per line; 0 means the seed is in no element.
    - `status`: `(S,)` int32, how each line ended: `MAX_STEPS` (it took `max_steps` steps), `LEFT` (a stage point has no
      element), `STALLED` (a stage speed is not `> min_speed`) or `OUTSIDE` (the seed has no element).  For
      `direction="both"` it is `(S, 2)`: the backward half, then the forward half.
    """

    def __init__(self, points: np.ndarray, n: np.ndarray, status: np.ndarray):
        self.points, self.n, self.status = points, n, status

    def lines(self):
        """A list of `(n_i, d)` arrays: the valid points of every line."""
        return [self.points[i, :int(c)].copy() for i, c in enumerate(self.n)]

    def lengths(self) -> np.ndarray:
        """`(S,)`: the length of each line's polyline (0.0 for a line of fewer than two points), added up on the host."""
        out = np.zeros(self.points.shape[0])
        for i, c in enumerate(self.n):
            if c >= 2:
                seg = np.diff(self.points[i, :int(c)], axis=0)
                out[i] = float(np.sum(np.sqrt(np.sum(seg * seg, axis=1))))
        return out


def join_both(back: Streamlines, fwd: Streamlines) -> Streamlines:
    """The `direction="both"` result from the two one-sided traces of the same seeds: per seed the backward line
    reversed and without its duplicate seed, then the forward line."""
    S, m1, d = fwd.points.shape
    points = np.full((S, 2 * m1 - 1, d), np.nan)
    n = np.zeros(S, dtype=np.int32)
    for i in range(S):
        nb, nf = int(back.n[i]), int(fwd.n[i])
        if nf == 0:                                        # the seed is in no element: neither half has a point
            continue
        points[i, :nb - 1] = back.points[i, nb - 1:0:-1]
        points[i, nb - 1:nb - 1 + nf] = fwd.points[i, :nf]
        n[i] = nb - 1 + nf
    return Streamlines(points, n, np.stack([back.status, fwd.status], axis=1).astype(np.int32))


def _field_kind(field) -> int:
    if not isinstance(field, str) or field not in _FIELDS:
        raise ValueError(f"StreamTracer: field must be 'vector' or 'gradient' (got {field!r})")
    return _FIELDS[field]


def _check_field(name: str, d: int, p: int, N: int, kind: int, z) -> np.ndarray:
    Z = np.asarray(z)
    if Z.dtype.kind not in "fiu":
        raise ValueError(f"StreamTracer: the field must be real numbers (got dtype {Z.dtype})")
    Z = np.asarray(Z, dtype=np.float64)
    want = (p * N, d) if kind == 0 else (p * N,)
    if Z.shape != want:
        what = "field='vector' needs the velocity components as columns" if kind == 0 else "field='gradient' needs u"
        raise ValueError(f"StreamTracer: {what}: shape {want} for this {name} geometry (got {Z.shape})")
    return Z


def _check_trace(d: int, seeds, step, max_steps, direction, normalize, min_speed):
    P = np.asarray(seeds)
    if P.dtype.kind not in "fiu":
        raise ValueError(f"StreamTracer.trace: seeds must be real numbers (got dtype {P.dtype})")
    P = np.asarray(P, dtype=np.float64)
    if P.ndim != 2 or P.shape[1] != d:
        raise ValueError(f"StreamTracer.trace: seeds must be (S, {d}) (got shape {P.shape})")
    try:
        step, min_speed = float(step), float(min_speed)
    except (TypeError, ValueError):
        raise ValueError("StreamTracer.trace: step and min_speed must be numbers") from None
    if not (math.isfinite(step) and step > 0.0):
        raise ValueError(f"StreamTracer.trace: step must be finite and positive (got {step})")
    if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 1:
        raise ValueError(f"StreamTracer.trace: max_steps must be an integer >= 1 (got {max_steps!r})")
    if not (math.isfinite(min_speed) and min_speed >= 0.0):
        raise ValueError(f"StreamTracer.trace: min_speed must be finite and >= 0 (got {min_speed})")
    if not isinstance(direction, str) or direction not in _DIRECTIONS:
        raise ValueError(f"StreamTracer.trace: direction must be 'forward', 'backward' or 'both' (got {direction!r})")
    if not isinstance(normalize, (bool, np.bool_)):
        raise ValueError(f"StreamTracer.trace: normalize must be True or False (got {normalize!r})")
    if P.shape[0] * (int(max_steps) + 1) * d >= 2 ** 31:
        raise ValueError(f"StreamTracer.trace: S * (max_steps + 1) * d = {P.shape[0]} * {int(max_steps) + 1} * {d} "
                         "exceeds 32-bit indexing (2**31)")
    return P, step, int(max_steps), min_speed


class StreamTracer(DeviceObject):
    """The field lines of `v = (z[:, 0], .., z[:, d-1])` (`field="vector"`: `z` is `(p*N, d)`, the columns are the
    velocity components) or of `v = grad u` (`field="gradient"`: `z` is `(p*N,)`), traced on the device.

    Supported: `fem2d` and `fem3d` (Q_k, `1 <= k <= 8`, curved elements included), `fem2d_P1`, `fem2d_P2` (curved
    elements when built with `curved=True`).  `fem1d`, embedded manifolds and the spectral families raise `ValueError`.  The node coordinates, the
    basis table, the location grid (cells, candidate lists, element boxes) and the field stay on the device for the life
    of the tracer; `set_field(z2)` replaces the field alone (the frames of a parabolic solve), `trace` may be called any
    number of times.

    The integrator is the classical Runge-Kutta scheme with the fixed step `h` (`step`, or `-step` backward), in this
    arithmetic (no fused multiply-add; tests/streamlines_twin.py restates it and the GPU tests compare bit for bit):

        k1 = v(x);  k2 = v(x + (0.5*h)*k1);  k3 = v(x + (0.5*h)*k2);  k4 = v(x + h*k3)
        x_new = x + (h/6.0)*(((k1 + 2.0*k2) + 2.0*k3) + k4)

    `v(y)` is bitwise `interpolate(geom, z, y)` (`field="vector"`) or the gradient of `interpolate(geom, u, y,
    gradient=True)`: the element of `y` is the lowest-index element of its grid cell's candidate list that contains it,
    never a warm start from the previous element, which would change the element a point on a shared face takes.  Every
    stage forms `speed = sqrt(v.v)` (squares added in axis order); with `normalize=True` the stage velocity is
    `v / speed`, so `step` is arc length.  A stage point without an element ends the line at the current `x` with `LEFT`
    (`OUTSIDE`, and no point, when it is the seed itself); `not speed > min_speed` ends it with `STALLED` (also NaN, and
    `0/0` under `normalize`).  There is no clipping of the last step to the boundary: a line's last point may lie
    outside the mesh.

    Use it as a context manager or call `close()`.
    """

    _closed_message = "StreamTracer: the tracer is closed"
    _destroy = "mgbhip_stream_destroy"

    def __init__(self, geom: Geometry, z, field: str = "vector", device_id: int = 0):
        self._family, self._name, self._d, k, self._p, self._N, xnodes, table = _raycast_plan(geom, "StreamTracer", curved_p2=True)
        self._kind = _field_kind(field)
        Z = _check_field(self._name, self._d, self._p, self._N, self._kind, z)
        from .device import _ptr
        xnodes, table, Z = _c_f64(xnodes), _c_f64(table), _c_f64(Z)
        self._create(device_id, "mgbhip_stream_create", self._family, self._d, k, self._p, self._N, _ptr(xnodes),
                     _ptr(table), self._kind, _ptr(Z))

    def set_field(self, z):
        """Replace the field by `z` (the shape the tracer was built with); the mesh and the grid stay resident."""
        self._open()
        Z = _c_f64(_check_field(self._name, self._d, self._p, self._N, self._kind, z))
        from .device import _check, _ptr
        _check(self._ctx.lib, self._ctx.lib.mgbhip_stream_set_field(self._handle, _ptr(Z)))

    def _trace_one(self, P: np.ndarray, h: float, max_steps: int, normalize: bool, min_speed: float) -> Streamlines:
        S = P.shape[0]
        points = np.full((S, max_steps + 1, self._d), np.nan)
        n, status = np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.int32)
        if S:
            from .device import ERR_INVALID, MGBHipError, _check, _ptr
            ip = C.POINTER(C.c_int32)
            try:
                _check(self._ctx.lib, self._ctx.lib.mgbhip_stream_trace(
                    self._handle, S, _ptr(P), h, max_steps, int(normalize), min_speed, _ptr(points),
                    n.ctypes.data_as(ip), status.ctypes.data_as(ip)))
            except MGBHipError as e:
                if e.status == ERR_INVALID:
                    raise ValueError(str(e)) from None
                raise
        return Streamlines(points, n, status)

    def trace(self, seeds, step, max_steps: int, direction: str = "forward", normalize: bool = False,
              min_speed: float = 0.0) -> Streamlines:
        """Trace one line from every row of `seeds` (`(S, d)`; a non-finite seed is simply outside the mesh).

        `step > 0` is the step of the integrator, `max_steps >= 1` the most steps a line takes.  `direction="forward"`
        traces with `step`, `"backward"` with `-step`; `"both"` runs both and joins them per seed on the host: the
        backward line reversed and without its duplicate seed, then the forward line, so `points` is
        `(S, 2*max_steps + 1, d)` and `status` `(S, 2)` (backward, forward).  `S * (max_steps + 1) * d >= 2**31` raises
        `ValueError` before anything is allocated.
        """
        self._open()
        P, step, max_steps, min_speed = _check_trace(self._d, seeds, step, max_steps, direction, normalize, min_speed)
        P = _c_f64(P)
        if direction == "forward":
            return self._trace_one(P, step, max_steps, bool(normalize), min_speed)
        back = self._trace_one(P, -step, max_steps, bool(normalize), min_speed)
        if direction == "backward":
            return back
        return join_both(back, self._trace_one(P, step, max_steps, bool(normalize), min_speed))


def streamlines(geom: Geometry, z, seeds, step, max_steps: int, field: str = "vector", direction: str = "forward",
                normalize: bool = False, min_speed: float = 0.0, device_id: int = 0) -> Streamlines:
    """Bitwise `StreamTracer(geom, z, field).trace(seeds, step, max_steps, direction, normalize, min_speed)`, with every
    argument checked before any device work."""
    _, name, d, _, p, N, _, _ = _raycast_plan(geom, "streamlines", curved_p2=True)
    _check_field(name, d, p, N, _field_kind(field), z)
    _check_trace(d, seeds, step, max_steps, direction, normalize, min_speed)
    with StreamTracer(geom, z, field, device_id=device_id) as st:
        return st.trace(seeds, step, max_steps, direction, normalize, min_speed)
