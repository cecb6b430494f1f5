"""polylines() without a GPU: the sequential twin (tests/polyline_twin.py) pinned on exact answers, the real curves checked
on the twins alone, and the host layer of mgb_amd.polyline (argument checks, resampling abscissae, save, segments)."""
import numpy as np
import pytest

import mgb_amd as m
import polyline_cases as K
from polyline_twin import polylines_twin, sample_twin


def assert_valid_walk(t, cells, S_edges):
    """Consecutive points share the named segment, lines end on -1 and every edge appears exactly once."""
    cells = np.asarray(cells)
    L = t.offsets.shape[0] - 1
    seen = []
    for l in range(L):
        o0, o1 = int(t.offsets[l]), int(t.offsets[l + 1])
        assert o1 - o0 >= 2 and t.segment[o1 - 1] == -1
        for j in range(o0, o1 - 1):
            s = int(t.segment[j])
            assert s >= 0 and {int(cells[s, 0]), int(cells[s, 1])} == {int(t.vertex[j]), int(t.vertex[j + 1])}
            seen.append(s)
        assert bool(t.closed[l]) == (t.vertex[o0] == t.vertex[o1 - 1] and _is_cycle(t, o0, o1, cells))
    assert len(seen) == len(set(seen)) == S_edges


def _is_cycle(t, o0, o1, cells):
    """The first vertex of the line has exactly two edges (a closed line passes through no node)."""
    v = t.vertex[o0]
    kept = np.unique(np.sort(cells[cells[:, 0] != cells[:, 1]], axis=1), axis=0)
    return int(np.sum(kept == v)) == 2


@pytest.mark.parametrize("name", sorted(K.EXACT))
def test_twin_on_exact_answers(name):
    X, cells = K.exact(name)
    t = polylines_twin(X, cells)
    offsets, vertex, segment, closed, ndropped = K.expected_arrays(name)
    assert np.array_equal(t.offsets, offsets) and t.offsets.dtype == np.int64
    assert np.array_equal(t.vertex, vertex) and np.array_equal(t.segment, segment)
    assert np.array_equal(t.closed, closed) and t.ndropped == ndropped
    assert_valid_walk(t, cells, cells.shape[0] - ndropped)
    X3, _ = K.exact(name, e=3)
    t3 = polylines_twin(X3, cells)
    assert np.array_equal(t3.vertex, vertex) and np.all(t3.arclength >= t.arclength)


def test_reversed_and_lines():
    X, cells = K.exact("y")
    pl = K.as_polylines(polylines_twin(X, cells), X, cells)
    assert pl.reversed().tolist() == [True, False, False, False, True, False]
    assert [ln.tolist() for ln in pl.lines()] == [X[[0, 3]].tolist(), X[[1, 3]].tolist(), X[[2, 3]].tolist()]
    X, cells = K.exact("lollipop_b")
    pl = K.as_polylines(polylines_twin(X, cells), X, cells)
    assert pl.reversed().tolist() == [False, False, True, True, True, False]
    assert pl.nlines == 2


def test_lengths_of_square_and_345_triangle():
    X, cells = K.unit_square()
    t = polylines_twin(X, cells)
    assert t.vertex.tolist() == [0, 1, 2, 3, 0] and t.closed.tolist() == [1]
    assert t.arclength.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and t.length.tolist() == [4.0]
    for e in (2, 3):
        X, cells = K.triangle_345(e)
        t = polylines_twin(X, cells)
        assert t.vertex.tolist() == [0, 1, 2, 0] and t.segment.tolist() == [1, 2, 0, -1]
        assert t.arclength.tolist() == [0.0, 3.0, 7.0, 12.0] and t.length.tolist() == [12.0]
    X, cells = K.zero_length_edge()
    t = polylines_twin(X, cells)
    assert t.arclength.tolist() == [0.0, 3.0, 3.0, 7.0]


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("S", [127, 128, 129])
def test_twin_on_shuffled_chains(S, closed):
    X, cells, order = K.chain(S, closed)
    t = polylines_twin(X, cells)
    if closed:
        i = int(np.argmin(order))
        ring = np.roll(order, -i)
        if ring[-1] < ring[1]:
            ring = np.roll(ring[::-1], 1)
        want = np.concatenate([ring, ring[:1]])
    else:
        want = order if order[0] < order[-1] else order[::-1]
    assert np.array_equal(t.vertex, want) and t.closed.tolist() == [int(closed)] and t.ndropped == 0
    assert_valid_walk(t, cells, S)


@pytest.mark.parametrize("nspirals", [1, 2])
def test_twin_on_spirals(nspirals):
    X, cells = K.spiral_mesh(nspirals)
    t = polylines_twin(X, cells)
    assert np.diff(t.offsets).tolist() == [4097] * nspirals and not t.closed.any() and t.ndropped == 0
    assert_valid_walk(t, cells, 4096 * nspirals)


@pytest.mark.parametrize("name", K.CLOSED)
def test_closed_real_curves_on_the_twins(name):
    mesh = K.real_mesh(name)
    assert np.all(mesh.vertex_valence() == 2) and not mesh.degenerate().any()
    t = polylines_twin(mesh.vertices, mesh.cells)
    assert t.closed.tolist() == [1, 1] and t.ndropped == 0
    assert int(t.offsets[-1]) == mesh.cells.shape[0] + 2
    assert_valid_walk(t, mesh.cells, mesh.cells.shape[0])
    level = mesh.level[t.segment[t.offsets[:-1]]]                             # one level per line, in launch order
    assert sorted(level.tolist()) == [0, 1]
    for l in range(2):
        assert np.all(mesh.level[t.segment[t.offsets[l]:t.offsets[l + 1] - 1]] == level[l])


@pytest.mark.parametrize("name", sorted(K.OPEN))
def test_open_real_curves_on_the_twins(name):
    _, S, V = K.OPEN[name]
    mesh = K.real_mesh(name)
    assert mesh.cells.shape == (S, 2) and mesh.vertices.shape == (V, 2)
    assert not mesh.degenerate().any() and mesh.edges()[0].shape[0] == S          # no degenerate, no duplicate segment
    assert np.sort(mesh.vertex_valence()).tolist() == [1] * 4 + [2] * (V - 4)    # four ends
    t = polylines_twin(mesh.vertices, mesh.cells)
    assert t.closed.tolist() == [0, 0] and t.ndropped == 0 and int(t.offsets[-1]) == S + 2
    assert_valid_walk(t, mesh.cells, S)
    assert np.array_equal(mesh.vertex_data[:, 0], mesh.vertices[:, 0])             # the carried field is x


@pytest.mark.parametrize("S", [1, 5, 126])
def test_boundary_loop_of_a_strip(S):
    X, cells = K.boundary_loop(S)
    t = polylines_twin(X, cells)
    assert t.closed.tolist() == [1] and np.diff(t.offsets).tolist() == [S + 3] and t.vertex[0] == 0
    assert_valid_walk(t, cells, S + 2)


# ---------------------------------------------------------------------------------------------------------------------
# the host layer
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "HipContext", boom)


def test_every_refusal_is_a_value_error_before_the_device(no_library):
    X, cells = K.exact("theta")
    tri = np.zeros((2, 3, 3))
    for bad, text in ((tri, "got ndarray"), (m.Tessellation(tri, np.zeros(2, np.int32), None), "Tessellation"),
                      (m.Contour(tri, np.zeros(2, np.int32), np.zeros(2, np.int32), None, 1), r"\(2, 3, 3\)"),
                      (K.W.as_mesh(_tiny_triangle_mesh()), "nv = 2"), ("curves", "got str"), ((X, cells, 1), "got tuple"),
                      ((X[:, :1], cells), "e in"), ((X, cells.reshape(-1)), r"cells must be \(S, 2\)"),
                      ((X, cells.astype(np.float64)), "integers"), ((X, cells + 1), r"\[0, V = 5\)"),
                      ((X, cells - 1), r"\[0, V = 5\)"), ((np.where(X == X[2, 1], np.inf, X), cells), "non-finite"),
                      ((object(), cells), "vertices must be")):
        with pytest.raises(ValueError, match="polylines: .*" + text):
            m.polylines(bad)
    with pytest.raises(ValueError, match="tol applies only"):
        m.polylines((X, cells), tol=1e-9)
    for tol in (-1.0, float("nan"), "x"):
        with pytest.raises(ValueError, match="weld: tol"):
            m.polylines(m.Contour(np.zeros((1, 2, 2)), np.zeros(1, np.int32), np.zeros(1, np.int32), None, 1), tol=tol)
    pl = K.as_polylines(polylines_twin(X, cells), X, cells)
    for line, s, text in ((3, 0.0, r"line must lie in \[0, 3\)"), (-1, 0.0, "line must lie"), (0, np.nan, "s must be finite"),
                          (0, np.inf, "s must be finite"), (0.5, 0.0, "line must be integers"),
                          ([0, 1], [0.0, 1.0, 2.0], "line and s do not broadcast")):
        with pytest.raises(ValueError, match="Polylines.at: " + text):
            pl.at(line, s)
    for kw, text in ((dict(), "exactly one"), (dict(n=3, spacing=0.1), "exactly one"), (dict(n=1), "n must be >= 2"),
                     (dict(n=2.5), "n must be an integer"), (dict(spacing=0.0), "spacing must be finite and > 0"),
                     (dict(spacing=float("inf")), "spacing must be finite"), (dict(spacing="h"), "spacing must be a number")):
        with pytest.raises(ValueError, match="resample: .*" + text):
            pl.resample(**kw)
    Xs, cs = K.unit_square()
    with pytest.raises(ValueError, match=">= 3 when a line is closed"):
        K.as_polylines(polylines_twin(Xs, cs), Xs, cs).resample(n=2)
    with pytest.raises(ValueError, match="suffix must be .obj or .vtk"):
        pl.save("lines.ply")


def _tiny_triangle_mesh():
    from weld_twin import weld_twin
    return weld_twin(K.W.two_triangles())


def test_empty_input_opens_no_handle(no_library):
    for curves, e in (((np.zeros((4, 3)), np.zeros((0, 2), np.int32)), 3), (np.zeros((0, 2, 2)), None)):
        if e is None:
            curves, e = m.Contour(curves, np.zeros(0, np.int32), np.zeros(0, np.int32), None, 2), 2
        pl = m.polylines(curves)
        assert pl.offsets.tolist() == [0] and pl.offsets.dtype == np.int64 and pl.nlines == 0 and pl.ndropped == 0
        assert pl.vertex.shape == pl.segment.shape == pl.arclength.shape == (0,) and pl.points.shape == (0, e)
        assert pl.closed.dtype == np.uint8 and pl.rounds == (0, 0) and pl.lines() == []
        assert pl.at(np.zeros(0, np.int32), np.zeros(0)).shape == (0, e)
        pts, off = pl.resample(n=4)
        assert pts.shape == (0, e) and off.tolist() == [0]
    assert m.polylines(m.Contour(np.zeros((0, 2, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32), None, 2)).mesh is not None


def test_resample_abscissae_and_counts():
    X, cells = K.zero_length_edge()                    # open, arclength 0, 3, 3, 7
    pl = K.as_polylines(polylines_twin(X, cells), X, cells)
    line, s, off = pl.abscissae(n=5)
    assert line.tolist() == [0] * 5 and off.tolist() == [0, 5] and s.tolist() == [0.0, 1.75, 3.5, 5.25, 7.0]
    line, s, off = pl.abscissae(spacing=2.0)            # ceil(3.5) + 1 = 5 points
    assert s.tolist() == [0.0, 1.75, 3.5, 5.25, 7.0]
    assert pl.abscissae(spacing=100.0)[1].tolist() == [0.0, 7.0]
    assert pl.abscissae(n=4)[1][-1] == 7.0 and pl.abscissae(n=4)[1][1] == 1 * (7.0 / 3)
    Xs, cs = K.unit_square()                            # closed, length 4
    sq = K.as_polylines(polylines_twin(Xs, cs), Xs, cs)
    line, s, off = sq.abscissae(n=8)
    assert s.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5] and off.tolist() == [0, 8]
    assert sq.abscissae(spacing=0.8)[1].tolist() == [i * (4.0 / 5) for i in range(5)]
    assert sq.abscissae(spacing=9.0)[1].tolist() == [i * (4.0 / 3) for i in range(3)]
    X, cells = K.exact("lollipop_a")                    # two lines: counts per line from their own lengths
    lo = K.as_polylines(polylines_twin(X, cells), X, cells)
    line, s, off = lo.abscissae(spacing=0.5)
    want = [max(2, int(np.ceil(ln / 0.5)) + 1) for ln in lo.length]
    assert np.diff(off).tolist() == want and np.bincount(line).tolist() == want
    assert s[off[1] - 1] == lo.length[0] and s[off[1]] == 0.0 and s[-1] == lo.length[1]
    # what the abscissae select, on the twin's sampler
    pts, _ = sample_twin(sq.points, None, sq.offsets, sq.arclength, 0, [0.0, 0.5, 1.0, 3.5, 4.0, 9.0, -1.0])
    assert pts.tolist() == [[0, 0], [0.5, 0], [1, 0], [0, 0.5], [0, 0], [0, 0], [0, 0]]
    pts, _ = sample_twin(pl.points, None, pl.offsets, pl.arclength, 0, [3.0, 2.9999999999999996, 5.0])
    assert pts[0].tolist() == [1.0, 2.0, 2.0] and pts[2].tolist() == [1.0, 2.0, 4.0] and pts[1, 2] < 2.0


def test_save_parses_back(tmp_path):
    mesh = K.real_mesh("open_P1")
    t = polylines_twin(mesh.vertices, mesh.cells)
    pl = K.as_polylines(t, mesh.vertices, mesh.cells, mesh.vertex_data)
    pl.level = mesh.level[t.segment[t.offsets[:-1]]]
    P, L = pl.points.shape[0], pl.nlines
    pl.save(tmp_path / "lines.obj")
    rows = [r.split() for r in open(tmp_path / "lines.obj").read().splitlines() if not r.startswith("#")]
    v = np.array([[float(x) for x in r[1:]] for r in rows if r[0] == "v"])
    ls = [[int(x) - 1 for x in r[1:]] for r in rows if r[0] == "l"]
    assert np.array_equal(v[:, :2], pl.points) and np.all(v[:, 2] == 0.0)
    assert ls == [list(range(pl.offsets[l], pl.offsets[l + 1])) for l in range(L)]
    pl.save(tmp_path / "lines.vtk")
    txt = open(tmp_path / "lines.vtk").read().splitlines()
    assert txt[3] == "DATASET POLYDATA" and txt[4] == "POINTS %d double" % P
    pts = np.array([[float(x) for x in r.split()] for r in txt[5:5 + P]])
    assert np.array_equal(pts[:, :2], pl.points)
    assert txt[5 + P] == "LINES %d %d" % (L, L + P)
    for l in range(L):
        row = [int(x) for x in txt[6 + P + l].split()]
        assert row[0] == len(row) - 1 and row[1:] == list(range(pl.offsets[l], pl.offsets[l + 1]))
    i = txt.index("SCALARS arclength double 1")
    assert np.array_equal(np.array([float(x) for x in txt[i + 2:i + 2 + P]]), pl.arclength)
    i = txt.index("SCALARS data0 double 1")
    assert np.array_equal(np.array([float(x) for x in txt[i + 2:i + 2 + P]]), pl.vertex_data[:, 0])
    i = txt.index("SCALARS level int 1")
    assert [int(x) for x in txt[i + 2:i + 2 + L]] == pl.level.tolist() and sorted(pl.level.tolist()) == [0, 1]
    i = txt.index("SCALARS closed int 1")
    assert [int(x) for x in txt[i + 2:i + 2 + L]] == [0, 0]


def test_segments_of_polylines():
    X, cells = K.exact("lollipop_a", e=3)
    pl = K.as_polylines(polylines_twin(X, cells), X, cells)
    pts, vals = m.segments(pl)
    assert vals is None and pts.shape == (4, 2, 3)
    assert np.array_equal(pts, np.stack([X[[0, 1, 2, 3]], X[[1, 2, 3, 1]]], axis=1))
    pts, vals = m.segments(pl, values=pl.arclength)
    assert np.array_equal(vals, np.stack([pl.arclength[[0, 2, 3, 4]], pl.arclength[[1, 3, 4, 5]]], axis=1))
    pl.vertex_data = np.stack([pl.vertex.astype(np.float64), np.zeros(6)], axis=1)
    assert m.segments(pl)[1].tolist() == [[0, 1], [1, 2], [2, 3], [3, 1]]
    with pytest.raises(ValueError, match="one per point"):
        m.segments(pl, values=np.zeros(4))
    flat = K.exact("lollipop_a")
    with pytest.raises(ValueError, match="not in R\\^3"):
        m.segments(K.as_polylines(polylines_twin(*flat), *flat))
    # in a list with what segments() already takes
    X2, c2 = K.exact("pair_ff", e=3)
    both, _ = m.segments([K.as_polylines(polylines_twin(X2, c2), X2, c2), pts[:1]])
    assert np.array_equal(both, np.concatenate([np.stack([X2[[0, 2]], X2[[2, 1]]], axis=1), pts[:1]]))
