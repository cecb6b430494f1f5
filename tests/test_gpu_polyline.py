"""polylines() on the device against the sequential twin (tests/polyline_twin.py), which walks the lines edge by edge.

`offsets`, `vertex`, `segment`, `closed` and `ndropped` are integers and `points` / `vertex_data` are gathers, so they are
compared with `np.array_equal`: no tolerance applies.  Arc length: the device adds the `k` edge lengths before point `k` of
a line in the order of its doubling tree and the twin as a running sum; two sums of the same `k` non-negative terms in
different orders differ by at most `2 (k - 1) eps` of the sum, and `6 eps` more allow a differently rounded square root,
so `|a_dev - a_twin| <= (2 k + 4) eps a_twin` (the largest observed error / bound is recorded).
Sampling runs the same IEEE operations in the same order as the twin's sampler given the device's own `arclength`, in a
file compiled without contraction, so `at()` and `resample()` are compared bitwise.
"""
import ctypes as C
import math

import numpy as np
import pytest

import mgb_amd as m
import polyline_cases as K
from helpers import record_observation
from polyline_twin import polylines_twin, sample_twin

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)


def assert_same(pl, X, cells, label, data=None, record=True):
    """The device result `pl` against the twin on `(X, cells)`: integers and gathers bitwise, arc length within its bound."""
    t = polylines_twin(X, cells)
    assert pl.offsets.dtype == np.int64 and pl.vertex.dtype == pl.segment.dtype == np.int32 and pl.closed.dtype == np.uint8
    assert np.array_equal(pl.offsets, t.offsets) and np.array_equal(pl.vertex, t.vertex)
    assert np.array_equal(pl.segment, t.segment) and np.array_equal(pl.closed, t.closed) and pl.ndropped == t.ndropped
    assert np.array_equal(pl.points, np.asarray(X)[t.vertex])
    if data is not None:
        assert np.array_equal(pl.vertex_data, data[t.vertex])
    k = np.arange(t.vertex.shape[0]) - np.repeat(t.offsets[:-1], np.diff(t.offsets))
    err = np.abs(pl.arclength - t.arclength)
    bound = (2 * k + 4) * EPS * t.arclength
    assert np.all(err <= bound), (label, float(err.max()))
    assert np.array_equal(pl.length, pl.arclength[pl.offsets[1:] - 1])
    assert np.all(pl.arclength[pl.offsets[:-1]] == 0.0)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    if record:
        record_observation(f"polylines arclength {label}: max error / bound {worst:.3g} over {err.size} points "
                           f"(bound (2 k + 4) eps a)")
    assert all(r >= 1 for r in pl.rounds)
    return t


def test_exact_cases():
    for name in sorted(K.EXACT):
        if name == "all_dropped":
            continue
        for e in (2, 3):
            X, cells = K.exact(name, e)
            pl = m.polylines((X, cells))
            assert_same(pl, X, cells, f"{name} e={e}", record=False)
            offsets, vertex, segment, closed, ndropped = K.expected_arrays(name)
            assert np.array_equal(pl.vertex, vertex) and np.array_equal(pl.segment, segment)
            assert np.array_equal(pl.closed, closed) and pl.ndropped == ndropped and pl.mesh is None
    X, cells = K.exact("all_dropped")
    pl = m.polylines((X, cells))
    assert pl.nlines == 0 and pl.offsets.tolist() == [0] and pl.vertex.shape == (0,) and pl.ndropped == 2
    X, cells = K.unit_square()
    pl = m.polylines((X, cells))
    assert pl.arclength.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0] and pl.length.tolist() == [4.0]
    X, cells = K.triangle_345()
    pl = m.polylines((X, cells))
    assert pl.arclength.tolist() == [0.0, 3.0, 7.0, 12.0] and pl.reversed().tolist() == [False] * 4


def rounds_bound(S):
    return 2 * math.ceil(math.log2(2 * S)) + 8


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("S", [127, 128, 129])              # 254, 256, 258 half-edges: either side of one block
def test_chains_at_block_edges(S, closed):
    for e in (2, 3):
        X, cells, _ = K.chain(S, closed, e=e)
        pl = m.polylines((X, cells))
        assert_same(pl, X, cells, f"chain S={S} closed={closed} e={e}")
        assert pl.nlines == 1 and pl.closed.tolist() == [int(closed)]
        assert len(pl.rounds) >= 1 and all(1 <= r <= rounds_bound(S) for r in pl.rounds)


@pytest.mark.parametrize("nspirals", [1, 2])
def test_long_chains_in_logarithmic_rounds(nspirals):
    soup, expected = K.W.spirals(nspirals)
    mesh = m.weld(soup, tol=0.0)
    assert np.array_equal(mesh.cells, expected)
    pl = m.polylines(mesh)
    assert pl.mesh is mesh
    assert_same(pl, mesh.vertices, mesh.cells, f"{nspirals} spiral(s)")
    assert np.diff(pl.offsets).tolist() == [4097] * nspirals and not pl.closed.any()
    S = soup.shape[0]
    record_observation(f"polylines rounds, {nspirals} spiral(s) of 4096 shuffled segments: {pl.rounds} "
                       f"(2 S = {2 * S} half-edges, bound {rounds_bound(S)})")
    # rules out a walk bound by the length of the line (4096 edges here)
    assert len(pl.rounds) >= 1 and all(1 <= r <= rounds_bound(S) for r in pl.rounds)


@pytest.mark.parametrize("name", K.CLOSED + tuple(sorted(K.OPEN)))
def test_real_curves(name):
    P, level, carried = K.real_soup(name, device=True)
    soup = m.Contour(P, level, np.zeros(P.shape[0], dtype=np.int32), carried, 2)
    pl = m.polylines(soup)                                       # welded first; the mesh is kept
    mesh = pl.mesh
    assert mesh is not None and mesh.cells.shape == P.shape[:2]
    assert_same(pl, mesh.vertices, mesh.cells, name, mesh.vertex_data)
    assert pl.nlines == 2 and pl.closed.tolist() == [int(name in K.CLOSED)] * 2 and pl.ndropped == 0
    assert np.array_equal(pl.level, level[pl.segment[pl.offsets[:-1]]]) and sorted(pl.level.tolist()) == [0, 1]
    if name in K.OPEN:
        assert mesh.cells.shape[0] == K.OPEN[name][1] and mesh.vertices.shape[0] == K.OPEN[name][2]
    again = m.polylines(mesh)                                    # the mesh itself gives the same lines
    assert np.array_equal(again.vertex, pl.vertex) and np.array_equal(again.arclength, pl.arclength)
    assert again.mesh is mesh and np.array_equal(again.vertex_data, pl.vertex_data)


@pytest.mark.parametrize("S", [1, 5, 126])                   # 3, 7 and 128 boundary edges
def test_boundary_loop_of_a_welded_strip(S):
    X, cells = K.boundary_loop(S, device=True)
    pl = m.polylines((X, cells))
    assert_same(pl, X, cells, f"strip S={S}")
    assert pl.closed.tolist() == [1] and np.diff(pl.offsets).tolist() == [S + 3] and pl.vertex[0] == 0


def test_streamlines_are_welded_first():
    pts = np.full((2, 5, 3), np.nan)
    pts[0, :4] = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [1, 1, 1]]
    pts[1, :3] = [[5, 5, 5], [6, 5, 5], [1, 1, 1]]
    pl = m.polylines(m.Streamlines(pts, np.array([4, 3], dtype=np.int32), np.zeros(2, dtype=np.int32)), tol=0.0)
    assert pl.vertex.tolist() == [0, 1, 2, 3, 5, 4] and pl.segment.tolist() == [0, 1, 2, 4, 3, -1]
    assert pl.arclength.tolist()[:4] == [0.0, 1.0, 2.0, 3.0] and pl.mesh.cells.shape == (5, 2)


def queries(pl):
    """Every line at s = 0, its length, the arc length of every point, mid-edge values and beyond both ends."""
    line, s = [], []
    for l in range(pl.nlines):
        a = pl.arclength[pl.offsets[l]:pl.offsets[l + 1]]
        mid = 0.5 * (a[:-1] + a[1:])
        sl = np.concatenate([[0.0, a[-1], -0.25, a[-1] + 1.0, 2.0 * a[-1] + 3.0], a, mid, np.nextafter(a, 0.0),
                             np.nextafter(a, np.inf)])
        line.append(np.full(sl.shape, l))
        s.append(sl)
    return np.concatenate(line).astype(np.int64), np.concatenate(s)


@pytest.mark.parametrize("name", ["curve_P1", "open_P2", "zero_length", "chain3d"])
def test_sampling_is_bitwise_the_twin(name):
    if name == "zero_length":
        X, cells = K.zero_length_edge()
        pl = m.polylines((X, cells))
        assert pl.arclength.tolist() == [0.0, 3.0, 3.0, 7.0]
        assert pl.at(0, [3.0, 5.0, 7.0, 8.0]).tolist() == [[1, 2, 2], [1, 2, 4], [1, 2, 6], [1, 2, 6]]
    elif name == "chain3d":
        X, cells, _ = K.chain(129, True, e=3)
        pl = m.polylines((X, cells))
    else:
        pl = m.polylines(K.real_mesh(name, device=True))
        assert pl.vertex_data is not None
    line, s = queries(pl)
    want, want_data = sample_twin(pl.points, pl.vertex_data, pl.offsets, pl.arclength, line, s)
    got = pl.at(line, s)
    if pl.vertex_data is None:
        assert np.array_equal(got, want)
    else:
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want_data)
        assert np.array_equal(got[1][:, 0], got[0][:, 0])        # the carried field is x, interpolated alike
    for kw in (dict(n=7), dict(spacing=float(pl.length.max()) / 9.5)):
        qline, qs, off = pl.abscissae(**kw)
        want, want_data = sample_twin(pl.points, pl.vertex_data, pl.offsets, pl.arclength, qline, qs)
        res = pl.resample(**kw)
        assert np.array_equal(res[0], want) and np.array_equal(res[1], off)
        if pl.vertex_data is not None:
            assert np.array_equal(res[2], want_data)
        for l in range(pl.nlines):                                # the first sample of a line is its first point
            assert np.array_equal(res[0][off[l]], pl.points[pl.offsets[l]])
            if not pl.closed[l]:
                assert np.array_equal(res[0][off[l + 1] - 1], pl.points[pl.offsets[l + 1] - 1])


def as_cycles(pl):
    """The lines of `pl` as a set of cyclic vertex sequences, each rotated to its lowest vertex and smaller neighbour."""
    return sorted(tuple(pl.vertex[pl.offsets[l]:pl.offsets[l + 1]].tolist()) for l in range(pl.nlines))


def test_determinism_and_reversal():
    mesh = K.real_mesh("curve_P2", device=True)
    a, b = m.polylines(mesh), m.polylines(mesh)
    for x, y in ((a.offsets, b.offsets), (a.vertex, b.vertex), (a.segment, b.segment), (a.closed, b.closed),
                 (a.arclength, b.arclength), (a.length, b.length), (a.points, b.points), (a.vertex_data, b.vertex_data)):
        assert np.array_equal(x, y)
    assert a.rounds == b.rounds and a.ndropped == b.ndropped
    # the segments reversed and permuted: the same lines as cyclic sequences (start and direction are canonical)
    rng = np.random.default_rng(3)
    perm = rng.permutation(mesh.cells.shape[0])
    cells = np.ascontiguousarray(mesh.cells[perm][:, ::-1])
    r = m.polylines((mesh.vertices, cells))
    assert as_cycles(r) == as_cycles(a) and r.closed.all()
    assert sorted(np.diff(r.offsets).tolist()) == sorted(np.diff(a.offsets).tolist())
    for l in range(r.nlines):                                    # and segment names the permuted segments
        seg = r.segment[r.offsets[l]:r.offsets[l + 1] - 1]
        assert np.array_equal(np.sort(cells[seg], axis=1),
                              np.sort(np.stack([r.vertex[r.offsets[l]:r.offsets[l + 1] - 1],
                                                r.vertex[r.offsets[l] + 1:r.offsets[l + 1]]], axis=1), axis=1))


def test_library_refusals_through_the_c_abi():
    """What the Python layer refuses first is refused by the library too, naming the argument."""
    from mgb_amd import device
    from mgb_amd.device import HipContext, _ptr
    ip, lp, bp = C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    ctx = HipContext(0)
    try:
        lib = ctx.lib
        X, cells = K.exact("theta", e=3)
        h, L, P, nd = C.c_void_p(), C.c_int64(-1), C.c_int64(-1), C.c_int64(-1)

        def create(V, e, x, S, c, out=True):
            rc = lib.mgbhip_polyline_create(ctx.handle, V, e, None if x is None else _ptr(x), S,
                                            None if c is None else c.ctypes.data_as(ip), C.byref(h) if out else None,
                                            C.byref(L), C.byref(P), C.byref(nd))
            return rc, lib.mgbhip_last_error().decode()
        bad_x = X.copy()
        bad_x[3, 2] = np.nan
        bad_c = cells.copy()
        bad_c[4, 1] = 5
        neg_c = cells.copy()
        neg_c[0, 0] = -1
        for args, text in (((5, 1, X, 6, cells), "e must be 2 or 3"), ((5, 4, X, 6, cells), "e must be 2 or 3"),
                           ((5, 3, None, 6, cells), "null vertices"), ((5, 3, X, 6, None), "null cells"),
                           ((5, 3, X, 2 ** 30, cells), "2 S >= 2^31"), ((5, 3, X, 6, bad_c), "cells lies outside [0, V)"),
                           ((5, 3, X, 6, neg_c), "cells lies outside [0, V)"),
                           ((5, 3, bad_x, 6, cells), "vertices has a non-finite coordinate"),
                           ((5, 3, X, 6, cells, False), "null output pointer")):
            rc, msg = create(*args)
            assert rc == device.ERR_INVALID and text in msg, (args[:2], msg)
        assert lib.mgbhip_polyline_destroy(None) == device.OK
        rc, _ = create(5, 3, X, 0, None)                         # S = 0: an empty result, not an error
        assert rc == device.OK and (L.value, P.value, nd.value) == (0, 0, 0)
        off = np.full(1, -1, dtype=np.int64)
        assert lib.mgbhip_polyline_fetch(h, off.ctypes.data_as(lp), None, None, None, None, None) == device.OK
        assert off.tolist() == [0] and lib.mgbhip_polyline_destroy(h) == device.OK
        rc, _ = create(5, 3, X, 6, cells)
        assert rc == device.OK and (L.value, P.value, nd.value) == (3, 9, 0)
        off, vert, seg = np.empty(4, np.int64), np.empty(9, np.int32), np.empty(9, np.int32)
        closed, arc, length = np.empty(3, np.uint8), np.empty(9), np.empty(3)
        fetch = lambda o: lib.mgbhip_polyline_fetch(h, o, vert.ctypes.data_as(ip), seg.ctypes.data_as(ip),     # noqa: E731
                                                    closed.ctypes.data_as(bp), _ptr(arc), _ptr(length))
        assert fetch(None) == device.ERR_INVALID and "null offsets" in lib.mgbhip_last_error().decode()
        assert fetch(off.ctypes.data_as(lp)) == device.OK
        assert vert.tolist() == K.expected_arrays("theta")[1].tolist()
        rounds, nph = (C.c_int32 * 8)(), C.c_int32(0)
        assert lib.mgbhip_polyline_rounds(h, None, C.byref(nph)) == device.ERR_INVALID
        assert lib.mgbhip_polyline_rounds(h, rounds, C.byref(nph)) == device.OK and nph.value >= 1
        assert lib.mgbhip_polyline_destroy(h) == device.OK

        pts = np.ascontiguousarray(X[vert])
        out = np.empty((2, 3))

        def sample(e=3, points=pts, offsets=off, arclength=arc, line=(0, 2), s=(0.5, 0.25), outp=out):
            ln, sv = np.array(line, dtype=np.int32), np.array(s, dtype=np.float64)
            rc = lib.mgbhip_polyline_sample(ctx.handle, e, 9, None if points is None else _ptr(points), 0, None, 3,
                                            None if offsets is None else offsets.ctypes.data_as(lp),
                                            None if arclength is None else _ptr(arclength), 2, ln.ctypes.data_as(ip),
                                            _ptr(sv), None if outp is None else _ptr(outp), None)
            return rc, lib.mgbhip_last_error().decode()
        short = off.copy()
        short[1] = 1
        nan_arc = arc.copy()
        nan_arc[4] = np.nan
        for kw, text in ((dict(e=4), "e must be 2 or 3"), (dict(points=None), "null points"), (dict(offsets=None), "null offsets"),
                         (dict(arclength=None), "null points or arclength"), (dict(outp=None), "out_points"),
                         (dict(line=(0, 3)), "line lies outside [0, L)"), (dict(line=(-1, 0)), "line lies outside [0, L)"),
                         (dict(s=(0.0, np.nan)), "s must be finite"), (dict(s=(np.inf, 0.0)), "s must be finite"),
                         (dict(offsets=short), "at least two points"), (dict(arclength=nan_arc), "arclength must be finite")):
            rc, msg = sample(**kw)
            assert rc == device.ERR_INVALID and text in msg, (kw, msg)
        rc, _ = sample()
        assert rc == device.OK
        assert np.array_equal(out, sample_twin(pts, None, off, arc, [0, 2], [0.5, 0.25])[0])
    finally:
        ctx.close()


def test_render_lines_takes_polylines():
    X, cells, _ = K.chain(40, True, e=3)
    pl = m.polylines((X, cells))
    pts = np.stack([pl.points[:-1], pl.points[1:]], axis=1)       # one closed line: every consecutive pair
    centre = X.mean(axis=0)
    cam = dict(eye=centre + np.array([3.0, -40.0, 12.0]), target=centre, size=(48, 32), radius=0.4)
    img, depth = m.render_lines(pl, values=pl.arclength, **cam)
    img2, depth2 = m.render_lines(pts, values=np.stack([pl.arclength[:-1], pl.arclength[1:]], axis=1), **cam)
    assert np.array_equal(img, img2) and np.array_equal(depth, depth2) and np.isfinite(depth).any()
