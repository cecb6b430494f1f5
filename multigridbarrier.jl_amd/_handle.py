"""The lifecycle every post-processing class shares (`PointLocator`, `RayCaster`, `TriangleCaster`, `SegmentCaster`,
`StreamTracer`, `FigureRenderer`, `Quadrature`, `Faces`, `ResidualEstimator`): one context of its own, one handle of the C ABI in it, `close()`, the context-manager
protocol and `__del__`.  The device layer is imported only when a handle is created, so an object that needs no device
(no points, no rays, an empty soup) needs no library either."""
from __future__ import annotations

import ctypes as C


class DeviceObject:
    # Class-level, so they are there first thing: __del__ runs even when a check of __init__ raises before anything exists.
    _handle = _ctx = None
    closed = False
    _closed_message = ""        # what a method raises after close(): "<Class>: the <thing> is closed"
    _destroy = ""               # the C entry point that frees the handle: "mgbhip_<thing>_destroy"

    def _create(self, device_id: int, create: str, *args, outputs=(), invalid_is_value_error: bool = False):
        """Open a context on `device_id` and call `create(ctx, *args, &handle, *outputs)` in it.  If that raises the context
        is closed again and nothing is kept; with `invalid_is_value_error` the library's invalid-argument status is raised
        as `ValueError` with the same text."""
        from .device import ERR_INVALID, HipContext, MGBHipError, _check
        self._ctx = HipContext(device_id)
        h = C.c_void_p()
        try:
            _check(self._ctx.lib, getattr(self._ctx.lib, create)(self._ctx.handle, *args, C.byref(h), *outputs))
        except Exception as e:
            self._ctx.close()
            self._ctx = None
            if invalid_is_value_error and isinstance(e, MGBHipError) and e.status == ERR_INVALID:
                raise ValueError(str(e)) from None
            raise
        self._handle = h

    def _open(self):
        if self.closed:
            raise ValueError(self._closed_message)

    def close(self):
        """Free the device state; calling it again does nothing."""
        self.closed = True
        if self._handle is not None:
            getattr(self._ctx.lib, self._destroy)(self._handle)
            self._handle = None
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
