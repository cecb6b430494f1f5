"""weld() on the device against the NumPy / SciPy twin (tests/weld_twin.py), which labels by a different algorithm.

`cells`, `first_corner`, `component` and `ncomponents` are integers and `vertices` / `vertex_data` are gathers, so they are
compared with `np.array_equal`: no tolerance applies.  Normals run the same IEEE operations in the same order on both
sides, so the expected difference is 0; the bound `8 eps * sum|n_f| / |sum n_f|` per vertex only allows for a differently
rounded square root or division (observed on MI355X: largest error / bound 0).
"""
import numpy as np
import pytest

import mgb_amd as m
import weld_cases as W
from helpers import record_observation
from weld_twin import default_tol, weld_twin

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


def assert_same(mesh, t, soup, data=None):
    """The device result `mesh` against the twin's `t`: integers and gathers bitwise."""
    assert mesh.cells.dtype == np.int32 and mesh.cells.shape == soup.shape[:2]
    assert np.array_equal(mesh.cells, t.cells)
    assert np.array_equal(mesh.first_corner, t.first_corner)
    assert np.array_equal(mesh.component, t.component) and mesh.ncomponents == t.ncomponents
    assert np.array_equal(mesh.vertices, t.vertices)
    assert np.array_equal(mesh.vertices, soup.reshape(-1, soup.shape[2])[mesh.first_corner])
    if data is not None:
        assert np.array_equal(mesh.vertex_data, t.vertex_data)
    assert mesh.rounds[0] >= 1 and mesh.rounds[1] >= 1


def assert_normals(mesh, t, label):
    zero = ~np.isfinite(t.normal_bound)
    assert np.array_equal(mesh.normals[zero], t.normals[zero])            # all zeros on both sides
    err = np.abs(mesh.normals - t.normals).max(axis=1)[~zero]
    bound = 8 * EPS * t.normal_bound[~zero]
    worst = float((err / bound).max()) if err.size else 0.0
    record_observation(f"weld normals {label}: max error / bound {worst:.3g} over {err.size} vertices "
                       f"(bound 8 eps sum|n_f| / |sum n_f|)")
    assert np.all(err <= bound), (label, worst)


# ---------------------------------------------------------------------------------------------------------------------
# real soups, cut on the device
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(W.REAL))
def test_real_soups(name):
    P, group, data = W.real_soup(name, device=True)
    expect = W.REAL[name][3]
    tri3 = P.shape[1:] == (3, 3)
    if group is not None:
        soup = m.Contour(P, group, np.zeros(P.shape[0], dtype=np.int32), data, len(W.REAL[name][2]))
    else:
        soup = m.Tessellation(P, np.zeros(P.shape[0], dtype=np.int32), data)
    mesh = m.weld(soup, normals=tri3)
    t = weld_twin(P, group=group, data=data, normals=tri3)
    assert mesh.tol == t.tol == default_tol(P)
    assert_same(mesh, t, P, data)
    if tri3:
        assert_normals(mesh, t, name)
    if group is not None:
        assert mesh.level is group
    # the properties themselves, on the device result
    assert not mesh.degenerate().any()
    assert mesh.is_closed() == expect["closed"] and mesh.boundary_edges().shape[0] == 0
    assert mesh.euler_characteristic().tolist() == expect["chi"]
    if P.shape[1] == 2:
        assert np.all(mesh.vertex_valence() == 2)


def test_exact_soups():
    soup = W.tetrahedron()
    mesh = m.weld(soup, normals=True)
    t = weld_twin(soup, normals=True)
    assert_same(mesh, t, soup)
    assert_normals(mesh, t, "tetrahedron")
    np.testing.assert_allclose(mesh.normals, mesh.vertices / np.sqrt(3.0), rtol=0, atol=4e-16)
    assert mesh.is_closed() and mesh.euler_characteristic().tolist() == [2]
    two = np.concatenate([soup, soup + 10.0])
    assert_same(m.weld(two), weld_twin(two), two)
    assert m.weld(two).ncomponents == 2
    flat = W.two_triangles()
    mesh = m.weld(flat)
    assert_same(mesh, weld_twin(flat), flat)
    assert mesh.boundary_edges().shape == (4, 2)
    tiny = np.nextafter(0.0, 1.0)
    zeros = np.array([[[0.0, 1.0], [-0.0, 1.0]], [[tiny, 1.0], [0.0, np.nextafter(1.0, 2.0)]]])
    assert m.weld(zeros, tol=0.0).cells.tolist() == [[0, 0], [1, 2]]


# ---------------------------------------------------------------------------------------------------------------------
# the smallest shapes at which the kernels can go wrong
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 127, 128, 129])          # M = 2, 254, 256, 258 corners: either side of one block
@pytest.mark.parametrize("e", [2, 3])
def test_segment_soups_at_block_edges(S, e):
    soup = W.polyline(S, e)
    data = np.arange(2.0 * S).reshape(S, 2)
    mesh = m.weld(soup, data=data)
    assert_same(mesh, weld_twin(soup, data=data), soup, data)
    assert mesh.vertices.shape[0] == S + 1 and mesh.ncomponents == 1


@pytest.mark.parametrize("S", [1, 85, 86])                 # M = 3, 255, 258 corners
def test_triangle_soups_at_block_edges(S):
    soup = W.triangle_strip(S)
    mesh = m.weld(soup, normals=True)
    t = weld_twin(soup, normals=True)
    assert_same(mesh, t, soup)
    assert_normals(mesh, t, f"strip S={S}")
    assert mesh.vertices.shape[0] == S + 2
    flat = np.ascontiguousarray(soup[:, :, :2])
    assert_same(m.weld(flat), weld_twin(flat), flat)


def test_pairs_that_straddle_cells():
    soup, tol = W.straddling_pairs()
    flat = soup.reshape(-1, 3)
    assert float(np.max(flat.max(0) - flat.min(0))) == 2.0          # so the cell side is tol = extent / 512
    assert W.cluster_separation(soup, 500, tol) > 4 * tol
    mesh = m.weld(soup, tol=tol)
    assert_same(mesh, weld_twin(soup, tol=tol), soup)
    assert mesh.vertices.shape[0] == 1500
    assert np.array_equal(mesh.cells[:500, 0], mesh.cells[500:, 0])           # every pair welds
    assert np.unique(mesh.cells[:500, 0]).size == 500                         # and no two pairs merge


def test_chains_across_cells():
    soup, tol = W.chain(0.9)
    mesh = m.weld(soup, tol=tol)
    assert_same(mesh, weld_twin(soup, tol=tol), soup)
    assert mesh.vertices.shape[0] == 65 and np.all(mesh.cells[:, 0] == 0) and mesh.first_corner[0] == 0
    assert np.array_equal(mesh.vertices[0], soup[0, 0])
    soup, tol = W.chain(1.1)
    mesh = m.weld(soup, tol=tol)
    assert_same(mesh, weld_twin(soup, tol=tol), soup)
    assert mesh.vertices.shape[0] == 128


def test_groups_keep_coincident_triangles_apart():
    a = W.tetrahedron()[:1]
    soup = np.concatenate([a, a])
    assert m.weld(soup).vertices.shape[0] == 3
    mesh = m.weld(soup, group=np.array([5, -2]))
    assert_same(mesh, weld_twin(soup, group=np.array([5, -2])), soup)
    assert mesh.cells.tolist() == [[0, 1, 2], [3, 4, 5]] and mesh.ncomponents == 2


def test_occupancy_guard_and_refusals():
    full = W.coincident(512)                                   # 1024 corners at one point: the cap itself
    mesh = m.weld(full)
    assert mesh.vertices.shape[0] == 1 and mesh.tol == 0.0 and mesh.degenerate().all()
    assert_same(mesh, weld_twin(full), full)
    assert m.weld(full, tol=0.25).vertices.shape[0] == 1
    with pytest.raises(ValueError, match=r"weld: 1026 corners fall into one grid cell with tol = 0\.5; at most "
                                         r"WELD_MAX_CELL = 1024"):
        m.weld(W.coincident(513), tol=0.5)
    with pytest.raises(ValueError, match="WELD_MAX_CELL = 1024"):         # a tolerance far too large for a real soup
        m.weld(W.polyline(600, 3), tol=1e6)
    soup = W.tetrahedron()
    bad = soup.copy()
    bad[1, 2, 1] = np.inf
    with pytest.raises(ValueError, match="non-finite coordinate"):
        m.weld(bad)
    for tol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="tol must be finite and >= 0"):
            m.weld(soup, tol=tol)
    with pytest.raises(ValueError, match="nv must be 2"):
        m.weld(np.zeros((2, 4, 3)))
    with pytest.raises(ValueError, match="normals need triangles"):
        m.weld(W.two_triangles(), normals=True)


def test_library_refusals_through_the_c_abi():
    """What the Python layer refuses first is refused by the library too, with the same text."""
    import ctypes as C
    from mgb_amd import device
    from mgb_amd.device import HipContext, _ptr
    ctx = HipContext(0)
    try:
        lib = ctx.lib
        P = np.ascontiguousarray(W.tetrahedron())
        h, V, nc = C.c_void_p(), C.c_int64(0), C.c_int64(0)

        def create(S, nv, e, pts, tol, normals):
            rc = lib.mgbhip_weld_create(ctx.handle, S, nv, e, _ptr(pts), None, tol, normals, C.byref(h), C.byref(V),
                                        C.byref(nc))
            return rc, lib.mgbhip_last_error().decode()
        for args, text in (((0, 3, 3, P, 0.0, 0), "no simplices"), ((4, 4, 3, P, 0.0, 0), "nv must be 2"),
                           ((4, 3, 1, P, 0.0, 0), "e must be 2 or 3"), ((2 ** 30, 2, 3, P, 0.0, 0), "M >= 2^31"),
                           ((4, 3, 3, P, -1.0, 0), "tol must be finite and >= 0"),
                           ((4, 3, 3, P, float("nan"), 0), "tol must be finite and >= 0"),
                           ((6, 2, 3, P, 0.0, 1), "normals need triangles")):
            rc, msg = create(*args)
            assert rc == device.ERR_INVALID and text in msg, (args[:3], msg)
        bad = P.copy()
        bad[0, 0, 0] = np.nan
        rc, msg = create(4, 3, 3, bad, 0.0, 0)
        assert rc == device.ERR_INVALID and "non-finite coordinate" in msg
        assert lib.mgbhip_weld_destroy(None) == device.OK
        rc, _ = create(4, 3, 3, P, 0.0, 1)
        assert rc == device.OK and V.value == 4 and nc.value == 1
        ip = C.POINTER(C.c_int32)
        cells, first, comp = np.empty(12, np.int32), np.empty(4, np.int32), np.empty(4, np.int32)
        assert lib.mgbhip_weld_fetch(h, cells.ctypes.data_as(ip), first.ctypes.data_as(ip), comp.ctypes.data_as(ip),
                                     None) == device.OK
        assert lib.mgbhip_weld_fetch(h, None, first.ctypes.data_as(ip), comp.ctypes.data_as(ip), None) == device.ERR_INVALID
        assert lib.mgbhip_weld_rounds(h, None, None) == device.ERR_INVALID
        assert lib.mgbhip_weld_destroy(h) == device.OK
    finally:
        ctx.close()


@pytest.mark.parametrize("nspirals", [1, 2])
def test_components_of_a_long_chain(nspirals):
    soup, expected = W.spirals(nspirals)
    mesh = m.weld(soup, tol=0.0)
    assert np.array_equal(mesh.cells, expected)                 # numbered by lowest corner, from the construction
    assert mesh.vertices.shape[0] == nspirals * 4097 and mesh.ncomponents == nspirals
    assert np.array_equal(mesh.component[mesh.cells[:, 0]], mesh.component[mesh.cells[:, 1]])
    assert np.all(mesh.vertex_valence() <= 2) and (mesh.vertex_valence() == 1).sum() == 2 * nspirals
    record_observation(f"weld rounds, {nspirals} spiral(s) of 4096 shuffled segments: vertex classes {mesh.rounds[0]}, "
                       f"components {mesh.rounds[1]} (V = {mesh.vertices.shape[0]}, log2 V = "
                       f"{np.log2(mesh.vertices.shape[0]):.1f})")
    # rules out propagation bound by the diameter (4096 edges here), which needs thousands of rounds
    assert 1 <= mesh.rounds[0] <= 256 and 1 <= mesh.rounds[1] <= 256


def test_determinism_and_reversal():
    P, group, data = W.real_soup("blobs_k2", device=True)
    a = m.weld(m.Contour(P, group, group, data, 3), normals=True)
    b = m.weld(m.Contour(P, group, group, data, 3), normals=True)
    for x, y in ((a.cells, b.cells), (a.first_corner, b.first_corner), (a.component, b.component),
                 (a.vertices, b.vertices), (a.normals, b.normals), (a.vertex_data, b.vertex_data)):
        assert np.array_equal(x, y)
    assert a.rounds == b.rounds and a.ncomponents == b.ncomponents
    # the simplices reversed: the same classes of corners, as a partition
    r = m.weld(np.ascontiguousarray(P[::-1]), group=np.ascontiguousarray(group[::-1]))
    assert r.vertices.shape[0] == a.vertices.shape[0] and r.ncomponents == a.ncomponents
    back = r.cells[::-1]                                        # the vertex (in r's numbering) of every corner of P
    pairs = np.unique(np.stack([a.cells.reshape(-1), back.reshape(-1)], axis=1), axis=0)
    assert pairs.shape[0] == a.vertices.shape[0]                # a bijection between the two numberings


def test_empty_soup_opens_no_handle(monkeypatch):
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "HipContext", boom)
    mesh = m.weld(np.zeros((0, 2, 3)))
    assert mesh.vertices.shape == (0, 3) and mesh.ncomponents == 0 and mesh.rounds == (0, 0)


def test_streamlines_weld_into_polylines():
    pts = np.full((2, 5, 3), np.nan)
    pts[0, :4] = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]]
    pts[1, :3] = [[5, 5, 5], [6, 5, 5], [1, 1, 1]]
    mesh = m.weld(m.Streamlines(pts, np.array([4, 3], dtype=np.int32), np.zeros(2, dtype=np.int32)), tol=0.0)
    assert mesh.cells.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5], [5, 3]] and mesh.ncomponents == 1
