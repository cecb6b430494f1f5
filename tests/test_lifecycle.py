"""The lifecycle the six post-processing classes share (mgb_amd._handle.DeviceObject), without a GPU: the library is
replaced by a stub that records the entry points called and answers with a chosen status.

For every class: the create call gets a context of its own and the class's create symbol; closing twice is silent and
calls the class's destroy symbol once, then closes the context; a method after `close()` raises the class's own
message; a create call that fails closes the context again, keeps nothing and raises; and `__del__` after an `__init__`
that raised, at an argument check or in the library, does not raise.
"""
import numpy as np
import pytest

import mgb_amd as m
from mgb_amd import device
from mgb_amd.figure import FigureRenderer
from mgb_amd.interpolate import PointLocator
from mgb_amd.raycast import RayCaster
from mgb_amd.streamlines import StreamTracer
from mgb_amd.surface import TriangleCaster
from mgb_amd.tubes import SegmentCaster


class StubLibrary:
    """Every entry point exists, records its name and returns `status[name]` (0: OK)."""

    def __init__(self):
        self.calls, self.status = [], {}

    def mgbhip_last_error(self):
        return b"stub: refused"

    def __getattr__(self, name):
        if not name.startswith("mgbhip_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return self.status.get(name, device.OK)
        return entry


@pytest.fixture
def stub(monkeypatch):
    lib = StubLibrary()

    class StubContext:
        def __init__(self, device_id=0, stream=None):
            self.lib, self.handle = lib, object()
            lib.calls.append("context")

        def close(self):
            if self.handle is not None:
                lib.calls.append("context closed")
                self.handle = None

    monkeypatch.setattr(device, "HipContext", StubContext)
    monkeypatch.setattr(device, "load_library", lambda: lib)
    return lib


GEOM3 = m.fem3d(k=1)
GEOM2 = m.fem2d(k=1)
O1, D1 = np.zeros((1, 3)), np.array([[0.0, 0.0, 1.0]])
TRI = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]])
SEG = np.array([[[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]])

# class -> (thing, good arguments, arguments an argument check refuses, a method that needs an open object)
CLASSES = {
    PointLocator: ("locator", lambda: ((GEOM2, np.zeros((1, 2))), {}), lambda: ((GEOM2, np.zeros((1, 3))), {}),
                   lambda x: x.evaluate(np.zeros(GEOM2.xflat.shape[0]))),
    RayCaster: ("raycast", lambda: ((GEOM3, O1, D1, 0.1), {}), lambda: ((GEOM3, O1, D1, -1.0), {}),
                lambda x: x.offsets),
    TriangleCaster: ("surface", lambda: ((TRI,), {}), lambda: ((np.zeros((1, 2, 3)),), {}), lambda x: x.trace(O1, D1)),
    SegmentCaster: ("tubes", lambda: ((SEG, 0.1), {}), lambda: ((SEG, -0.1), {}), lambda x: x.trace(O1, D1)),
    StreamTracer: ("stream", lambda: ((GEOM3, np.zeros((GEOM3.xflat.shape[0], 3))), {}),
                   lambda: ((GEOM3, np.zeros(5)), {}), lambda x: x.set_field(np.zeros((GEOM3.xflat.shape[0], 3)))),
    FigureRenderer: ("figure", lambda: ((GEOM3, (3.0, 2.0, 1.0), (0.0, 0.0, 0.0)), dict(size=(4, 3), isosurfaces=[0.5], clim=(0.0, 1.0))),
                     lambda: ((GEOM3, (3.0, 2.0, 1.0), (0.0, 0.0, 0.0)), dict(size=(4, 3), isosurfaces=[0.5], clim=None)),
                     lambda x: x.render(np.zeros(GEOM3.xflat.shape[0]))),
}
CLOSED = {PointLocator: "PointLocator: the locator is closed", RayCaster: "RayCaster: the caster is closed",
          TriangleCaster: "TriangleCaster: the caster is closed", SegmentCaster: "SegmentCaster: the caster is closed",
          StreamTracer: "StreamTracer: the tracer is closed", FigureRenderer: "FigureRenderer: the renderer is closed"}
CREATE = {"locator": "mgbhip_locator_create", "raycast": "mgbhip_raycast_create", "surface": "mgbhip_surface_create",
          "tubes": "mgbhip_tubes_create", "stream": "mgbhip_stream_create", "figure": "mgbhip_figure_create"}
IDS = [c.__name__ for c in CLASSES]


@pytest.mark.parametrize("cls", list(CLASSES), ids=IDS)
def test_close_twice_is_silent_and_a_method_after_it_raises(stub, cls):
    thing, good, _, method = CLASSES[cls]
    args, kwargs = good()
    obj = cls(*args, **kwargs)
    assert stub.calls == ["context", CREATE[thing]] and not obj.closed
    obj.close()
    assert obj.closed and stub.calls[2:] == [f"mgbhip_{thing}_destroy", "context closed"]
    obj.close()
    obj.__del__()
    assert len(stub.calls) == 4, "the second close and __del__ call nothing"
    with pytest.raises(ValueError) as e:
        method(obj)
    assert str(e.value) == CLOSED[cls]
    assert len(stub.calls) == 4
    with cls(*args, **kwargs) as again:
        assert not again.closed
    assert again.closed and stub.calls[4:] == ["context", CREATE[thing], f"mgbhip_{thing}_destroy", "context closed"]


@pytest.mark.parametrize("cls", list(CLASSES), ids=IDS)
def test_del_after_a_refused_argument_does_not_raise(stub, cls):
    bad = CLASSES[cls][2]
    args, kwargs = bad()
    obj = cls.__new__(cls)
    with pytest.raises(ValueError):
        obj.__init__(*args, **kwargs)
    assert stub.calls == [], "refused before the library is touched"
    obj.close()                                            # what __del__ runs, without its catch-all
    obj.__del__()
    assert stub.calls == [] and obj.closed


@pytest.mark.parametrize("cls", list(CLASSES), ids=IDS)
def test_del_after_a_failed_create_does_not_raise(stub, cls):
    thing, good, _, _ = CLASSES[cls]
    stub.status[CREATE[thing]] = device.ERR_INVALID
    args, kwargs = good()
    obj = cls.__new__(cls)
    with pytest.raises((ValueError, device.MGBHipError), match="stub: refused"):
        obj.__init__(*args, **kwargs)
    assert stub.calls == ["context", CREATE[thing], "context closed"], "the context of a failed create is closed again"
    obj.close()
    obj.__del__()
    assert len(stub.calls) == 3, "nothing is left to destroy"
