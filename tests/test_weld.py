"""weld() on the CPU: the NumPy / SciPy twin (tests/weld_twin.py) the GPU tests compare against is itself checked on
exact answers, the soups of tests/test_gpu_weld.py are checked on the twin alone (closed, Euler characteristic, valence),
every Python-side refusal fires before the library is touched, and `IndexedMesh.save()` round-trips.
"""
import numpy as np
import pytest

import mgb_amd as m
import weld_cases as W
from weld_twin import default_tol, weld_twin


# ---------------------------------------------------------------------------------------------------------------------
# the twin on exact answers
# ---------------------------------------------------------------------------------------------------------------------

def test_weld_is_exported():
    from mgb_amd.weld import weld, IndexedMesh
    assert m.weld is weld and m.IndexedMesh is IndexedMesh


def test_tetrahedron():
    soup = W.tetrahedron()
    t = weld_twin(soup, normals=True)
    mesh = W.as_mesh(t)
    assert t.vertices.shape == (4, 3) and t.ncomponents == 1
    assert mesh.is_closed() and mesh.boundary_edges().shape == (0, 2)
    assert mesh.euler_characteristic().tolist() == [2]
    assert not mesh.degenerate().any()
    e, valence = mesh.edges()
    assert e.shape == (6, 2) and np.all(valence == 2)
    # outward normals: the vertices are (+-1, +-1, +-1), so the normal at p is p / sqrt(3)
    np.testing.assert_allclose(t.normals, t.vertices / np.sqrt(3.0), rtol=0, atol=4e-16)
    # numbered by lowest corner, nothing averaged
    assert np.array_equal(t.vertices, soup.reshape(-1, 3)[t.first_corner])
    assert np.all(np.diff(t.first_corner) > 0) and t.first_corner[0] == 0
    assert np.array_equal(t.cells.reshape(-1)[t.first_corner], np.arange(4))


def test_two_triangles_sharing_an_edge():
    mesh = W.as_mesh(weld_twin(W.two_triangles()))
    assert mesh.vertices.shape == (4, 2)
    e, valence = mesh.edges()
    assert e.shape == (5, 2) and sorted(valence.tolist()) == [1, 1, 1, 1, 2]
    assert mesh.boundary_edges().shape == (4, 2) and not mesh.is_closed()
    assert mesh.euler_characteristic().tolist() == [1]


def test_square_polyline():
    mesh = W.as_mesh(weld_twin(W.square_polyline()))
    assert mesh.vertices.shape == (4, 2) and mesh.ncomponents == 1
    assert mesh.vertex_valence().tolist() == [2, 2, 2, 2]
    assert mesh.is_closed() and mesh.euler_characteristic().tolist() == [0]
    open_line = W.as_mesh(weld_twin(W.polyline(5)))
    assert not open_line.is_closed() and open_line.boundary_edges().shape == (2, 2)
    assert open_line.euler_characteristic().tolist() == [1]


def test_two_far_apart_copies_are_two_components():
    a = W.tetrahedron()
    t = weld_twin(np.concatenate([a, a + 10.0]))
    assert t.vertices.shape[0] == 8 and t.ncomponents == 2
    assert t.component.tolist() == [0, 0, 0, 0, 1, 1, 1, 1]
    assert W.as_mesh(t).euler_characteristic().tolist() == [2, 2]


def test_groups_keep_coincident_corners_apart():
    a = W.two_triangles()[:1]
    soup = np.concatenate([a, a])
    assert weld_twin(soup).vertices.shape[0] == 3
    t = weld_twin(soup, group=np.array([0, 1]))
    assert t.vertices.shape[0] == 6 and t.ncomponents == 2
    assert t.cells.tolist() == [[0, 1, 2], [3, 4, 5]]


def test_zero_tolerance_welds_signed_zeros_and_nothing_else():
    tiny = np.nextafter(0.0, 1.0)
    soup = np.array([[[0.0, 1.0], [-0.0, 1.0]], [[tiny, 1.0], [0.0, np.nextafter(1.0, 2.0)]]])
    t = weld_twin(soup, tol=0.0)
    assert t.cells.tolist() == [[0, 0], [1, 2]]
    assert W.as_mesh(t).degenerate().tolist() == [True, False]


def test_chains_weld():
    soup, tol = W.chain(0.9)
    t = weld_twin(soup, tol=tol)
    assert t.vertices.shape[0] == 1 + 64 and np.all(t.cells[:, 0] == 0) and t.first_corner[0] == 0
    soup, tol = W.chain(1.1)
    assert weld_twin(soup, tol=tol).vertices.shape[0] == 128


def test_straddling_pairs_input_and_twin():
    soup, tol = W.straddling_pairs()
    flat = soup.reshape(-1, 3)
    assert float(np.max(flat.max(0) - flat.min(0))) == 2.0 and tol == 2.0 / 512
    assert W.cluster_separation(soup, 500, tol) > 4 * tol
    near = soup[:, 0]
    assert np.all(np.abs(near[:500] - near[500:]).max(-1) == pytest.approx(0.5 * tol, rel=1e-9))
    # about half the pairs per axis sit in different cells of side tol
    cell = np.floor((near - flat.min(0)) / tol)
    split = (cell[:500] != cell[500:]).mean(axis=0)
    assert np.all(split > 0.15) and np.all(split < 0.85), split
    t = weld_twin(soup, tol=tol)
    assert t.vertices.shape[0] == 1500
    assert np.array_equal(t.cells[:500, 0], t.cells[500:, 0])
    assert np.unique(t.cells[:500, 0]).size == 500


def test_spiral_construction_agrees_with_the_twin():
    soup, expected = W.spirals(2, nseg=512)
    t = weld_twin(soup, tol=0.0)
    assert np.array_equal(t.cells, expected) and t.ncomponents == 2
    assert W.as_mesh(t).vertex_valence().max() == 2


# ---------------------------------------------------------------------------------------------------------------------
# the GPU cases, on the twin alone
# ---------------------------------------------------------------------------------------------------------------------

_twin_cache = {}


def twin_of(name):
    if name not in _twin_cache:
        P, group, data = W.real_soup(name)
        assert P.shape[0] * P.shape[1] <= 6000, name
        _twin_cache[name] = (P, group, weld_twin(P, group=group, data=data, normals=P.shape[1:] == (3, 3)))
    return _twin_cache[name]


@pytest.mark.parametrize("name", sorted(W.REAL))
def test_real_soups_on_the_twin(name):
    P, group, t = twin_of(name)
    expect = W.REAL[name][3]
    mesh = W.as_mesh(t, level=group)
    print(f"{name}: S = {P.shape[0]}, V = {t.vertices.shape[0]}, components = {t.ncomponents}, tol = {t.tol:.3e}")
    assert t.tol == default_tol(P)
    assert not mesh.degenerate().any()
    assert mesh.is_closed() == expect["closed"]
    assert mesh.euler_characteristic().tolist() == expect["chi"]
    if P.shape[1] == 2:
        assert np.all(mesh.vertex_valence() == 2)
    if group is not None:                      # every component lies in one level group
        comp_of_simplex = t.component[t.cells[:, 0]]
        for c in range(t.ncomponents):
            assert np.unique(group[comp_of_simplex == c]).size == 1


def test_sphere_vertex_counts_are_recorded():
    """The figures behind DESIGN section 8: V of the three sphere isosurfaces at the default tolerance."""
    assert [twin_of(n)[2].vertices.shape[0] for n in ("sphere_k1", "sphere_k2", "sphere_k3")] == [14, 146, 74]


def test_copies_are_far_closer_than_distinct_vertices():
    """The default tolerance sits between the two scales on every real soup: the welded classes have a diameter below
    2^-40 of the extent, and distinct vertices are at least 2^-20 of the extent apart."""
    for name in sorted(W.REAL):
        P, group, t = twin_of(name)
        X = P.reshape(-1, P.shape[2])
        ext = t.tol * 2.0 ** 27
        spread = np.abs(X - t.vertices[t.cells.reshape(-1)]).max()
        D = np.abs(t.vertices[:, None] - t.vertices[None]).max(-1)
        same = np.eye(D.shape[0], dtype=bool)
        if group is not None:
            g = np.asarray(group)[t.first_corner // P.shape[1]]
            same |= g[:, None] != g[None, :]
        gap = D[~same].min()
        print(f"{name}: copies within {spread / ext:.2e} of the extent, distinct vertices {gap / ext:.2e} apart")
        assert spread <= 2.0 ** -40 * ext and gap >= 2.0 ** -20 * ext


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: ValueError before any device work
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library or open a device context fails the test."""
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "load_library", boom)
    monkeypatch.setattr(device, "HipContext", boom)


def test_refusals_fire_before_the_device(no_library):
    tri, seg = W.tetrahedron(), W.square_polyline()
    with pytest.raises(ValueError, match=r"weld: the soup must be \(S, nv, e\)"):
        m.weld(np.zeros((4, 3)))
    with pytest.raises(ValueError, match="weld: the soup must be a Contour"):
        m.weld("soup")
    with pytest.raises(ValueError, match=r"weld: nv must be 2 \(segments\) or 3 \(triangles\)"):
        m.weld(np.zeros((2, 4, 3)))
    for e in (1, 4):
        with pytest.raises(ValueError, match="weld: e must be 2 or 3"):
            m.weld(np.zeros((2, 3, e)))
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="weld: tol must be finite and >= 0"):
            m.weld(tri, tol=bad)
    with pytest.raises(ValueError, match="weld: tol must be a number or None"):
        m.weld(tri, tol="1e-9")
    for soup in (seg, W.polyline(3, e=3), W.two_triangles()):
        with pytest.raises(ValueError, match=r"weld: normals need triangles in R\^3"):
            m.weld(soup, normals=True)
    for bad in (np.zeros(3, dtype=np.int32), np.zeros((4, 1), dtype=np.int32), np.zeros(4)):
        with pytest.raises(ValueError, match=r"weld: group must be \(4,\) integers"):
            m.weld(tri, group=bad)
    for bad in (np.zeros(4), np.zeros((4, 2)), np.zeros((3, 3, 1))):
        with pytest.raises(ValueError, match=r"weld: data must be \(4, 3\) or \(4, 3, C\)"):
            m.weld(tri, data=bad)
    for bad in (np.nan, np.inf, -np.inf):
        soup = tri.copy()
        soup[2, 1, 0] = bad
        with pytest.raises(ValueError, match="weld: a corner has a non-finite coordinate"):
            m.weld(soup)


def test_empty_soup_needs_no_library(no_library):
    mesh = m.weld(np.zeros((0, 3, 3)), normals=True, data=np.zeros((0, 3, 2)))
    assert mesh.vertices.shape == (0, 3) and mesh.cells.shape == (0, 3) and mesh.cells.dtype == np.int32
    assert mesh.first_corner.shape == (0,) and mesh.component.shape == (0,) and mesh.ncomponents == 0
    assert mesh.normals.shape == (0, 3) and mesh.vertex_data.shape == (0, 2) and mesh.rounds == (0, 0)
    assert not mesh.is_closed() and mesh.euler_characteristic().shape == (0,)
    assert mesh.edges()[0].shape == (0, 2) and mesh.boundary_edges().shape == (0, 2)
    empty = m.Contour(np.zeros((0, 2, 2)), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), None, 3)
    mesh = m.weld(empty)
    assert mesh.cells.shape == (0, 2) and mesh.level is empty.level and mesh.tol == 0.0
    lines = m.Streamlines(np.full((2, 4, 3), np.nan), np.array([0, 1], dtype=np.int32), np.zeros(2, dtype=np.int32))
    assert m.weld(lines).cells.shape == (0, 2)


def test_streamlines_become_segments():
    from mgb_amd.weld import _check
    pts = np.full((2, 4, 2), np.nan)
    pts[0, :3] = [[0, 0], [1, 0], [1, 1]]
    pts[1, :2] = [[5, 5], [6, 5]]
    P = _check(m.Streamlines(pts, np.array([3, 2], dtype=np.int32), np.zeros(2, dtype=np.int32)), None, False, None, None)[0]
    assert P.tolist() == [[[0, 0], [1, 0]], [[1, 0], [1, 1]], [[5, 5], [6, 5]]]


# ---------------------------------------------------------------------------------------------------------------------
# save(): the text parses back to the mesh
# ---------------------------------------------------------------------------------------------------------------------

def _parse_obj(path):
    v, vn, cells = [], [], []
    for ln in open(path).read().splitlines():
        w = ln.split()
        if not w or w[0] == "#":
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] in ("l", "f"):
            cells.append([int(x.split("/")[0]) - 1 for x in w[1:]])
            if "//" in w[1]:
                assert all(x.split("//")[0] == x.split("//")[1] for x in w[1:])
    return np.array(v), np.array(vn), np.array(cells)


def _parse_vtk(path):
    tok = open(path).read().split("\n")
    assert tok[0].startswith("# vtk DataFile") and tok[2] == "ASCII" and tok[3] == "DATASET POLYDATA"
    out, i = {}, 4
    while i < len(tok):
        w = tok[i].split()
        i += 1
        if not w:
            continue
        if w[0] == "POINTS":
            n = int(w[1])
            out["points"] = np.array([[float(x) for x in tok[i + j].split()] for j in range(n)])
            i += n
        elif w[0] in ("LINES", "POLYGONS"):
            n = int(w[1])
            rows = [[int(x) for x in tok[i + j].split()] for j in range(n)]
            assert int(w[2]) == sum(len(r) for r in rows) and all(r[0] == len(r) - 1 for r in rows)
            out["kind"], out["cells"] = w[0], np.array([r[1:] for r in rows])
            i += n
        elif w[0] in ("CELL_DATA", "POINT_DATA"):
            where, count = w[0], int(w[1])
        elif w[0] == "SCALARS":
            assert tok[i] == "LOOKUP_TABLE default"
            conv = int if w[2] == "int" else float
            out[(where, w[1])] = np.array([conv(tok[i + 1 + j]) for j in range(count)])
            i += 1 + count
        elif w[0] == "NORMALS":
            out[(where, "normals")] = np.array([[float(x) for x in tok[i + j].split()] for j in range(count)])
            i += count
        else:
            raise AssertionError(f"unexpected line {tok[i - 1]!r}")
    return out


@pytest.mark.parametrize("kind", ["triangles", "segments"])
def test_save_round_trips(tmp_path, kind):
    if kind == "triangles":
        soup = W.tetrahedron() * np.array([1.0 / 3.0, np.pi, np.e])
        t = weld_twin(soup, normals=True, data=np.arange(24.0).reshape(4, 3, 2) / 7.0)
        level = np.array([0, 0, 1, 1], dtype=np.int32)
    else:
        soup = W.square_polyline() / 3.0
        t = weld_twin(soup, data=np.arange(8.0).reshape(4, 2) / 3.0)
        level = None
    mesh = W.as_mesh(t, level=level)
    P3 = mesh.vertices if kind == "triangles" else np.concatenate([mesh.vertices, np.zeros((4, 1))], axis=1)

    mesh.save(tmp_path / "mesh.obj")
    v, vn, cells = _parse_obj(tmp_path / "mesh.obj")
    assert np.array_equal(v, P3) and np.array_equal(cells, mesh.cells)          # %.17g gives the doubles back
    if kind == "triangles":
        assert np.array_equal(vn, mesh.normals)
    else:
        assert vn.size == 0

    mesh.save(str(tmp_path / "mesh.VTK"))
    got = _parse_vtk(tmp_path / "mesh.VTK")
    assert np.array_equal(got["points"], P3) and np.array_equal(got["cells"], mesh.cells)
    assert got["kind"] == ("POLYGONS" if kind == "triangles" else "LINES")
    assert np.array_equal(got[("POINT_DATA", "component")], mesh.component)
    for j in range(mesh.vertex_data.shape[1]):
        assert np.array_equal(got[("POINT_DATA", f"data{j}")], mesh.vertex_data[:, j])
    if kind == "triangles":
        assert np.array_equal(got[("CELL_DATA", "level")], level)
        assert np.array_equal(got[("POINT_DATA", "normals")], mesh.normals)
    else:
        assert not any(k[0] == "CELL_DATA" for k in got if isinstance(k, tuple))

    with pytest.raises(ValueError, match="the suffix must be .obj or .vtk"):
        mesh.save(tmp_path / "mesh.ply")
