"""interpolate(..., gradient=True) on the CPU: the argument errors of the value path raised before any device work, the
exported entry point, and the shapes of empty results."""
import os
import re
import subprocess

import numpy as np
import pytest

import mgb_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nvals(geom):
    return geom.x.shape[0] * geom.x.shape[1]


GEOMS = [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.fem2d(k=2), "fem2d"),
    (m.fem3d(k=1), "fem3d"),
    (m.fem2d_P1(), "fem2d_P1"),
    (m.fem2d_P2(), "fem2d_P2"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
]


@pytest.mark.parametrize("geom,name", GEOMS)
def test_wrong_length_raises_before_device_work(geom, name):
    n = _nvals(geom)
    d = geom.x.shape[2]
    pts = 0.1 if d == 1 else np.zeros((2, d))
    with pytest.raises(ValueError, match=rf"^{name} interpolation needs {n} values \(got {n + 1}\)$"):
        m.interpolate(geom, np.zeros(n + 1), pts, gradient=True)
    with pytest.raises(ValueError, match=rf"needs {n} values \(got {n - 1}\)"):
        m.interpolate(geom, np.zeros((n - 1, 3)), pts, gradient=True, return_element=True)
    with pytest.raises(ValueError, match="vector or a matrix"):
        m.interpolate(geom, np.zeros((n, 1, 1)), pts, gradient=True)


@pytest.mark.parametrize("geom", [m.fem2d(k=1), m.fem3d(k=1), m.fem2d_P1(), m.fem2d_P2(), m.spectral2d(n=4)])
def test_point_width_must_be_d(geom):
    d = geom.x.shape[2]
    z = np.zeros(_nvals(geom))
    for bad in (np.zeros((3, d + 1)), np.zeros(d + 1), np.zeros((2, 3, d)), 0.5):
        with pytest.raises(ValueError, match=rf"M-by-{d} array"):
            m.interpolate(geom, z, bad, gradient=True)


def test_unsupported_geometries_are_refused():
    seg = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)
    with pytest.raises(ValueError, match="embedded manifolds"):
        m.interpolate(seg, np.zeros(_nvals(seg)), np.zeros((1, 2)), gradient=True)
    K = m.fem2d_P2().x.copy()
    K[6, 0, 0] += 1e-9 * (1 + abs(K[6, 0, 0]))
    curved = m.fem2d_P2(K=K)
    with pytest.raises(ValueError, match="straight elements"):
        m.interpolate(curved, np.zeros(_nvals(curved)), np.zeros((1, 2)), gradient=True)
    bad = m.fem2d_P1(K=m.fem2d_P1().x.copy())
    bad.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node"):
        m.interpolate(bad, np.zeros(_nvals(bad)), np.zeros((1, 2)), gradient=True)


def test_library_exports_and_header_declares_the_entry():
    from mgb_amd import device
    lib = device.load_library()
    assert hasattr(lib, "mgbhip_interpolate_grad")
    assert "mgbhip_interpolate_grad" in device.EXPORTS
    assert len(lib.mgbhip_interpolate_grad.argtypes) == len(lib.mgbhip_interpolate.argtypes) + 1
    hdr = open(os.path.join(ROOT, "include", "mgbhip.h")).read()
    assert re.search(r"\bint\s+mgbhip_interpolate_grad\s*\(", hdr)
    # exported symbols are exactly the declared ones
    declared = sorted(set(re.findall(r"\b(mgbhip_[a-z0-9_]+)\s*\(", hdr)))
    out = subprocess.run(["nm", "-D", "--defined-only", device.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if re.search(r"\sT\smgbhip_[a-z0-9_]+$", ln)})
    assert exported == declared


@pytest.mark.parametrize("geom,name", GEOMS)
def test_no_points_gives_empty_arrays_of_the_right_shape(geom, name):
    n = _nvals(geom)
    d = geom.x.shape[2]
    empty = np.zeros(0) if d == 1 else np.zeros((0, d))
    tail = () if d == 1 else (d,)
    vals, grads = m.interpolate(geom, np.zeros(n), empty, gradient=True)
    assert vals.shape == (0,) and grads.shape == (0,) + tail and grads.dtype == np.float64
    vals, grads, elem = m.interpolate(geom, np.zeros((n, 3)), empty, gradient=True, return_element=True)
    assert vals.shape == (0, 3) and grads.shape == (0, 3) + tail
    assert elem.shape == (0,) and elem.dtype == np.int32
    # the default is the old result: no tuple
    assert m.interpolate(geom, np.zeros(n), empty).shape == (0,)
    assert m.interpolate(geom, np.zeros(n), empty, gradient=False).shape == (0,)
