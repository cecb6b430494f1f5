"""PointLocator on the CPU: the entry points exist in the header, the symbol list and the library; the constructor and
`evaluate` raise what `interpolate()` raises; a locator of zero points works without a device; closing."""
import os
import re
import subprocess

import numpy as np
import pytest

import mgb_amd as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["mgbhip_locator_create", "mgbhip_locator_elements", "mgbhip_locator_evaluate", "mgbhip_locator_destroy"]

GEOMS = [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.fem2d(k=2), "fem2d"),
    (m.fem3d(k=1), "fem3d"),
    (m.fem2d_P1(), "fem2d_P1"),
    (m.fem2d_P2(), "fem2d_P2"),
    (m.fem2d_P2(bubble=False), "fem2d_P2"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
]


def _nvals(geom):
    return geom.x.shape[0] * geom.x.shape[1]


def _empty(geom):
    d = geom.x.shape[2]
    return np.zeros(0) if d == 1 else np.zeros((0, d))


def test_point_locator_is_exported():
    from mgb_amd.interpolate import PointLocator
    assert m.PointLocator is PointLocator


def test_entry_points_are_declared_listed_and_exported():
    from mgb_amd import device
    hdr = open(os.path.join(ROOT, "include", "mgbhip.h")).read()
    assert re.search(r"typedef\s+struct\s+mgbhip_locator\s+mgbhip_locator\s*;", hdr)
    lib = device.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", device.library_path()], capture_output=True, text=True,
                         check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if re.search(r"\sT\smgbhip_[a-z0-9_]+$", ln)}
    for name in SYMBOLS:
        assert re.search(rf"\bint\s+{name}\s*\(", hdr), name
        assert name in device.EXPORTS, name
        assert name in exported, name
        assert getattr(lib, name).argtypes is not None, name
    # create takes the arguments of mgbhip_interpolate without ncomp, z, out, elem and with the handle's address
    assert len(lib.mgbhip_locator_create.argtypes) == len(lib.mgbhip_interpolate.argtypes) - 3


@pytest.mark.parametrize("geom,name", GEOMS)
def test_wrong_z_is_refused_by_evaluate_with_interpolates_message(geom, name):
    n = _nvals(geom)
    with m.PointLocator(geom, _empty(geom)) as loc:
        with pytest.raises(ValueError, match=rf"^{name} interpolation needs {n} values \(got {n + 1}\)$"):
            loc.evaluate(np.zeros(n + 1))
        with pytest.raises(ValueError, match=rf"needs {n} values \(got {n - 1}\)"):
            loc.evaluate(np.zeros((n - 1, 3)), gradient=True)
        with pytest.raises(ValueError, match="z has no columns"):
            loc.evaluate(np.zeros((n, 0)))
        with pytest.raises(ValueError, match="z must be a vector or a matrix"):
            loc.evaluate(np.zeros((n, 1, 1)))
    for bad, pattern in ((np.zeros(n + 1), "needs"), (np.zeros((n, 0)), "no columns"), (np.zeros((n, 1, 1)), "vector or a matrix")):
        with pytest.raises(ValueError, match=pattern):
            m.interpolate(geom, bad, _empty(geom))


@pytest.mark.parametrize("geom", [m.fem2d(k=1), m.fem3d(k=1), m.fem2d_P1(), m.fem2d_P2(), m.spectral2d(n=4)])
def test_point_width_must_be_d(geom):
    d = geom.x.shape[2]
    for bad in (np.zeros((3, d + 1)), np.zeros(d + 1), np.zeros((2, 3, d)), 0.5):
        with pytest.raises(ValueError, match=rf"M-by-{d} array"):
            m.PointLocator(geom, bad)
        with pytest.raises(ValueError, match=rf"M-by-{d} array"):
            m.interpolate(geom, np.zeros(_nvals(geom)), bad)


def test_degree_out_of_range_is_refused():
    geom = m.fem1d(nodes=np.linspace(-1, 1, 3), k=9)
    with pytest.raises(ValueError, match=r"element degree k = 9 is outside 1\.\.8"):
        m.PointLocator(geom, np.zeros(2))
    with pytest.raises(ValueError, match=r"element degree k = 9 is outside 1\.\.8"):
        m.interpolate(geom, np.zeros(_nvals(geom)), np.zeros(2))


def test_embedded_manifold_is_refused():
    geom = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)     # a segment in the plane
    with pytest.raises(ValueError, match="embedded manifolds"):
        m.PointLocator(geom, np.zeros((1, 2)))


@pytest.mark.parametrize("bubble", [True, False])
def test_curved_p2_is_refused(bubble):
    geom = m.fem2d_P2(bubble=bubble)
    K = geom.x.copy()
    slot = 6 if bubble else 3
    K[slot, 0, 0] += 1e-9 * (1 + abs(K[slot, 0, 0]))      # one edge (or the bubble) node off its straight position
    with pytest.raises(ValueError, match="straight elements"):
        m.PointLocator(m.fem2d_P2(bubble=bubble, K=K), np.zeros((1, 2)))


def test_nonfinite_mesh_is_refused():
    geom = m.fem2d_P1(K=m.fem2d_P1().x.copy())
    geom.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node"):
        m.PointLocator(geom, np.zeros((1, 2)))
    with pytest.raises(ValueError, match="non-finite node"):       # checked before the point count, as in interpolate()
        m.PointLocator(geom, np.zeros((0, 2)))


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("geom,name", GEOMS)
def test_no_points_gives_what_interpolate_gives(geom, name):
    n = _nvals(geom)
    empty = _empty(geom)
    with m.PointLocator(geom, empty) as loc:
        assert loc.n_points == 0 and not loc.closed
        for z in (np.zeros(n), np.zeros((n, 3)), np.zeros((n, 1))):
            v0, e0 = m.interpolate(geom, z, empty, return_element=True)
            assert _same(loc.evaluate(z), v0)
            assert _same(loc.elements, e0) and loc.elements.dtype == np.int32
            v1, g1 = m.interpolate(geom, z, empty, gradient=True)
            v, g = loc.evaluate(z, gradient=True)
            assert _same(v, v1) and _same(g, g1)
    assert loc.closed


def test_closed_locator_refuses_and_close_is_idempotent():
    geom = m.fem2d_P1()
    loc = m.PointLocator(geom, np.zeros((0, 2)))
    assert loc.closed is False
    loc.close()
    assert loc.closed is True
    loc.close()                                                    # a second close does nothing
    with pytest.raises(ValueError, match="closed"):
        loc.evaluate(np.zeros(_nvals(geom)))
    with pytest.raises(ValueError, match="closed"):
        loc.elements
    with m.PointLocator(geom, np.zeros((0, 2))) as inner:
        pass
    assert inner.closed
    inner.close()
