"""StreamTracer / streamlines on the CPU: the NumPy twin (tests/streamlines_twin.py) on exact fields, the join rule of
`direction="both"`, and every argument check raised before the library is touched.  The cases of
tests/test_gpu_streamlines.py (meshes, fields, seeds) are defined here.

The bound of the closed-form tests.  One RK4 step forms four stage points `x + c k` (two roundings each, relative to
`max|x|`), the sum `((k1 + 2 k2) + 2 k3) + k4` (three roundings; the doublings are exact), its product with `h/6` and the
final sum (one rounding of the size of `x`): about `12 eps max|x|` in all, for fields with `|v| <= max|x|`.  A stage
velocity that an element evaluates as a sum over its `P` nodes carries at most about `P eps max|v|`, and the step
multiplies the four of them by `h/6 (1 + 2 + 2 + 1) = h`: `4 P h eps max|x|` with the intermediate stages counted
generously.  The errors of earlier steps are carried along by a factor `1 + O(h)` per step, which the generous constant
covers for the few dozen steps used here.  So `n` steps stay within `n (12 + 4 P h) eps max|x| <= 64 (n + 1) eps
max(1, max|x|)` while `P h <= 10`.  The exact fields of this file have no evaluation error (`P = 0`).
"""
import numpy as np
import pytest

import sys

import mgb_amd as m
from mgb_amd.streamlines import StreamTracer, Streamlines, join_both, streamlines
from streamlines_twin import LEFT, MAX_STEPS, OUTSIDE, STALLED, TwinLines, join_twin, trace_twin

sl = sys.modules["mgb_amd.streamlines"]          # the package attribute of that name is the function
EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble


def bound(n, xmax):
    return 64 * (n + 1) * EPS * max(1.0, xmax)


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_streamlines.py
# ---------------------------------------------------------------------------------------------------------------------

def curved_hex():
    """One curved Q_2 hexahedron: the unit cube's nodes bulged in +z by 0.1 (1 - x^2)(1 - y^2)(z + 1)/2."""
    X = m.fem3d(k=2).x.copy()
    x, y, z = X[..., 0].copy(), X[..., 1].copy(), X[..., 2].copy()
    X[..., 2] = z + 0.1 * (1 - x * x) * (1 - y * y) * (z + 1) / 2
    return m.fem3d(k=2, K=X)


# subdivide(geom, L) refines L - 1 times: subdivided twice is L = 3 (16 squares, 32 triangles), once is L = 2
GPU_CASES = {
    "fem2d_k1": lambda: m.subdivide(m.fem2d(k=1), 3),
    "fem2d_k2": lambda: m.subdivide(m.fem2d(k=2), 2),
    "fem2d_P1": lambda: m.subdivide(m.fem2d_P1(), 3),
    "fem2d_P2": lambda: m.subdivide(m.fem2d_P2(), 2),
    "fem3d_k1": lambda: m.subdivide(m.fem3d(k=1), 2),
    "fem3d_k2_curved": curved_hex,
}
GPU_MAX_STEPS = 24
GPU_STEP = {False: 0.07, True: 0.03}         # by normalize: with it the step is arc length, and every line would leave
GPU_MIN_SPEED = 0.3


def vector_field(X):
    """(n, d): a smooth non-polynomial field that turns about the origin, where it vanishes."""
    x, y = X[:, 0], X[:, 1]
    if X.shape[1] == 2:
        return np.stack([-y + 0.25 * np.sin(2.0 * x), x + 0.25 * np.sin(2.0 * y)], axis=1)
    z = X[:, 2]
    return np.stack([-y + 0.25 * np.sin(2.0 * x), x + 0.25 * np.sin(2.0 * y), -0.5 * z + 0.2 * np.sin(x * y)], axis=1)


def scalar_field(X):
    """(n,): a smooth non-polynomial saddle; its gradient vanishes near (-0.69, 0.23) and points out of the mesh along x."""
    x, y = X[:, 0], X[:, 1]
    u = 0.2 * (x * x - y * y) + 0.3 * np.sin(1.5 * x + 0.5 * y)
    if X.shape[1] == 3:
        u = u + 0.15 * X[:, 2] * X[:, 2]
    return u


def gpu_seeds(d, S):
    """(S, d): seeds on shared faces, edges and vertices of the meshes above, on the boundary, outside, one NaN and one
    Inf seed, then pseudo-random ones in [-1.2, 1.2]^d (about a third of them outside in 3-D)."""
    special2 = [(0.0, 0.0), (0.5, 0.5), (-0.5, 0.25), (0.25, 0.25), (0.0, 0.7), (-1.0, -1.0), (1.0, 0.25), (0.5, -1.0),
                (1.5, 0.0), (0.0, -1.0000001), (np.nan, 0.1), (0.2, np.inf), (0.02, -0.01), (0.75, 0.5),
                (-0.69, 0.23), (-0.66, 0.2), (-0.72, 0.26), (0.05, 0.03), (-0.04, 0.06)]
    sp = np.array([s + (0.0,) * (d - 2) for s in special2])
    if d == 3:
        sp = np.concatenate([sp, np.array([[0.0, 0.0, 0.5], [0.5, 0.0, -0.5], [0.3, -0.2, 1.0], [0.1, 0.1, 1.08],
                                           [0.0, 0.0, 1.2], [0.5, 0.5, 0.5]])])
    rnd = np.random.default_rng(1234 + d).uniform(-1.2, 1.2, size=(S - len(sp), d))
    return np.concatenate([sp, rnd])


# ---------------------------------------------------------------------------------------------------------------------
# the twin on exact fields
# ---------------------------------------------------------------------------------------------------------------------

def everywhere(f):
    return lambda P: (f(P), np.ones(len(P), dtype=bool))


def in_box(f, lo=-1.0, hi=1.0):
    return lambda P: (f(P), np.all((P >= lo) & (P <= hi), axis=1))


SEEDS2 = np.array([[0.3, -0.2], [-0.7, 0.45], [0.0, 0.9], [0.123456789, 0.987654321], [-0.5, -0.5]])


@pytest.mark.parametrize("h", [0.05, -0.05, 0.3])
def test_constant_field(h):
    c = np.array([0.6, -0.35, 0.2])
    seeds = np.concatenate([SEEDS2, np.linspace(-0.4, 0.4, 5)[:, None]], axis=1)
    n = 24
    t = trace_twin(everywhere(lambda P: np.tile(c, (len(P), 1))), seeds, h, n)
    assert np.array_equal(t.n, np.full(5, n + 1)) and np.array_equal(t.status, np.full(5, MAX_STEPS))
    for i in range(n + 1):
        want = seeds + (i * h) * c
        err = np.abs(t.points[:, i] - want).max()
        assert err <= bound(i, np.abs(want).max()), (i, err)


@pytest.mark.parametrize("h", [0.05, -0.05, 0.3])
def test_rotation(h):
    n = 32
    t = trace_twin(everywhere(lambda P: np.stack([-P[:, 1], P[:, 0]], axis=1)), SEEDS2, h, n)
    assert np.array_equal(t.n, np.full(5, n + 1))
    hl = LD(h)
    c, s = 1 - hl * hl / 2 + hl ** 4 / 24, hl - hl ** 3 / 6          # R(h) = I + hA + h^2A^2/2 + h^3A^3/6 + h^4A^4/24
    R = np.array([[c, -s], [s, c]], dtype=LD)
    rho = np.sqrt(c * c + s * s)
    want = SEEDS2.astype(LD)
    r0 = np.sqrt(np.sum(want * want, axis=1))
    for i in range(n + 1):
        err = float(np.abs(t.points[:, i].astype(LD) - want).max())
        xmax = float(np.abs(want).max())
        assert err <= bound(i, xmax), (i, err)
        radius = np.sqrt(np.sum(t.points[:, i].astype(LD) ** 2, axis=1))
        assert float(np.abs(radius - rho ** i * r0).max()) <= 2 * bound(i, xmax), i
        want = want @ R.T


@pytest.mark.parametrize("h", [0.04, -0.04])
def test_gradient_of_half_x_dot_x(h):
    n = 24
    seeds = np.concatenate([SEEDS2, np.linspace(-0.4, 0.4, 5)[:, None]], axis=1)
    t = trace_twin(everywhere(lambda P: P.copy()), seeds, h, n)
    assert np.array_equal(t.n, np.full(5, n + 1))
    hl = LD(h)
    g = 1 + hl + hl * hl / 2 + hl ** 3 / 6 + hl ** 4 / 24           # the scalar closed form of one step, per axis
    want = seeds.astype(LD)
    for i in range(n + 1):
        err = float(np.abs(t.points[:, i].astype(LD) - want).max())
        assert err <= bound(i, float(np.abs(want).max())), (i, err)
        want = want * g


@pytest.mark.parametrize("normalize", [False, True])
def test_zero_field_stalls_at_the_seed(normalize):
    t = trace_twin(everywhere(lambda P: np.zeros_like(P)), SEEDS2, 0.1, 8, normalize=normalize)
    assert np.array_equal(t.n, np.ones(5)) and np.array_equal(t.status, np.full(5, STALLED))
    assert np.array_equal(t.points[:, 0], SEEDS2) and np.isnan(t.points[:, 1:]).all()
    # NaN velocities stall, too
    t = trace_twin(everywhere(lambda P: np.full_like(P, np.nan)), SEEDS2, 0.1, 8, normalize=normalize)
    assert np.array_equal(t.n, np.ones(5)) and np.array_equal(t.status, np.full(5, STALLED))


def test_normalize_gives_equal_chords():
    c = np.array([3.0, -4.0])
    h, n = 0.0625, 16
    t = trace_twin(everywhere(lambda P: np.tile(c, (len(P), 1))), SEEDS2, h, n, normalize=True)
    chords = np.sqrt(np.sum(np.diff(t.points, axis=1) ** 2, axis=2))
    assert np.abs(chords - h).max() <= 16 * EPS * 2.0
    u = np.sqrt(np.sum(np.diff(SEEDS2, axis=0) ** 2, axis=1))           # nothing of the seeds' spacing leaks in
    assert u.min() > 0
    assert np.abs(t.points[:, n] - (SEEDS2 + n * h * c / 5.0)).max() <= bound(n, 2.0)


def test_statuses_and_the_points_they_leave():
    rot = in_box(lambda P: np.stack([-P[:, 1], P[:, 0]], axis=1))
    seeds = np.array([[0.5, 0.0], [0.98, 0.9], [0.0, 0.01], [1.5, 0.0], [np.nan, 0.0], [np.inf, 0.0]])
    t = trace_twin(rot, seeds, 0.1, 12, min_speed=0.05)
    assert list(t.status) == [MAX_STEPS, LEFT, STALLED, OUTSIDE, OUTSIDE, OUTSIDE]
    assert t.n[0] == 13 and 1 <= t.n[1] < 13 and t.n[2] == 1 and list(t.n[3:]) == [0, 0, 0]
    for i in range(6):
        assert np.isfinite(t.points[i, :t.n[i]]).all() and np.isnan(t.points[i, t.n[i]:]).all()
    assert np.isnan(t.points[3:]).all()
    assert np.array_equal(t.points[:3, 0], seeds[:3])
    # a line that leaves keeps its last point, which is the one outside (no clipping), or ends at a stage that left
    last = t.points[1, t.n[1] - 1]
    assert np.all(np.abs(t.points[1, :t.n[1] - 1]) <= 1.0) and np.isfinite(last).all()


def test_both_join_rule():
    rot = in_box(lambda P: np.stack([-P[:, 1], P[:, 0]], axis=1))
    seeds = np.array([[0.5, 0.0], [0.98, 0.9], [0.0, 0.01], [1.5, 0.0]])
    n = 12
    f, b = trace_twin(rot, seeds, 0.1, n, min_speed=0.05), trace_twin(rot, seeds, -0.1, n, min_speed=0.05)
    j = join_twin(b, f)
    assert j.points.shape == (4, 2 * n + 1, 2) and j.status.shape == (4, 2)
    assert np.array_equal(j.status[:, 0], b.status) and np.array_equal(j.status[:, 1], f.status)
    assert np.array_equal(j.n, [2 * n + 1, b.n[1] + f.n[1] - 1, 1, 0])
    assert np.array_equal(j.points[0, :n], b.points[0, :0:-1]) and np.array_equal(j.points[0, n:], f.points[0])
    assert np.array_equal(j.points[0, n], seeds[0]) and np.array_equal(j.points[2, 0], seeds[2])
    assert np.isnan(j.points[3]).all() and np.isnan(j.points[2, 1:]).all()
    # the module joins by the same rule
    mj = join_both(Streamlines(b.points, b.n, b.status), Streamlines(f.points, f.n, f.status))
    assert np.array_equal(mj.points, j.points, equal_nan=True) and np.array_equal(mj.n, j.n)
    assert np.array_equal(mj.status, j.status) and mj.n.dtype == np.int32 and mj.status.dtype == np.int32
    lines = mj.lines()
    assert [len(x) for x in lines] == list(j.n) and np.array_equal(lines[0], j.points[0])
    L = mj.lengths()
    assert L[2] == 0.0 and L[3] == 0.0
    assert abs(L[0] - np.sum(np.sqrt(np.sum(np.diff(j.points[0], axis=0) ** 2, axis=1)))) <= 64 * EPS


def test_backward_is_forward_of_the_negated_field():
    f = in_box(lambda P: np.stack([-P[:, 1] + 0.25 * np.sin(2 * P[:, 0]), P[:, 0]], axis=1))
    g = in_box(lambda P: -np.stack([-P[:, 1] + 0.25 * np.sin(2 * P[:, 0]), P[:, 0]], axis=1))
    a, b = trace_twin(f, SEEDS2, -0.1, 16, min_speed=0.1), trace_twin(g, SEEDS2, 0.1, 16, min_speed=0.1)
    assert np.array_equal(a.points, b.points, equal_nan=True) and np.array_equal(a.n, b.n)
    assert np.array_equal(a.status, b.status)


def test_names_and_constants_are_exported():
    assert m.StreamTracer is StreamTracer and m.streamlines is streamlines and m.Streamlines is Streamlines
    assert (sl.MAX_STEPS, sl.LEFT, sl.STALLED, sl.OUTSIDE) == (0, 1, 2, 3) == (MAX_STEPS, LEFT, STALLED, OUTSIDE)
    assert isinstance(TwinLines(None, None, None), TwinLines)


def test_gpu_seeds_cover_the_special_places():
    for d in (2, 3):
        for S in (65, 257):
            P = gpu_seeds(d, S)
            assert P.shape == (S, d)
            fin = np.isfinite(P).all(axis=1)
            assert (~fin).sum() == 2 and np.isnan(P).any() and np.isinf(P).any()
            assert (np.abs(P[fin]).max(axis=1) > 1.0).sum() >= 5, "seeds outside the mesh"
            assert (P[fin] == 0.0).all(axis=1).any() and (P[fin] == 0.5).all(axis=1).any(), "seeds on shared vertices"
        # the 65 seeds are the first 65 of the 257: the GPU tests compute the twin once, on the 257
        assert np.array_equal(gpu_seeds(d, 257)[:65], gpu_seeds(d, 65), equal_nan=True)


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


def _n(geom):
    return geom.x.shape[0] * geom.x.shape[1]


@pytest.mark.parametrize("geom,name", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
])
def test_unsupported_families_are_refused_by_name(no_library, geom, name):
    d = geom.xflat.shape[1]
    n = geom.xflat.shape[0]
    with pytest.raises(ValueError, match=rf"StreamTracer: {name} geometries are not supported"):
        StreamTracer(geom, np.zeros((n, d)))
    with pytest.raises(ValueError, match=rf"streamlines: {name} geometries are not supported"):
        streamlines(geom, np.zeros((n, d)), np.zeros((1, d)), step=0.1, max_steps=4)


def test_embedded_manifold_is_refused(no_library):
    geom = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)     # a segment in the plane
    with pytest.raises(ValueError, match=r"StreamTracer: fem1d embedded in 2 dimensions"):
        StreamTracer(geom, np.zeros((_n(geom), 2)))


def test_curved_p2_is_refused(no_library):
    K = m.fem2d_P2().x.copy()
    K[1, 0, :] += 0.05                                                     # an edge node off its edge's midpoint
    geom = m.fem2d_P2(K=K)
    with pytest.raises(ValueError, match=r"fem2d_P2 .* straight elements"):
        StreamTracer(geom, np.zeros((_n(geom), 2)))


def test_bad_fields_are_refused(no_library):
    geom = m.fem2d(k=1)
    n = _n(geom)
    for z in (np.zeros(n), np.zeros((n, 3)), np.zeros((n + 1, 2)), np.zeros((n, 2, 1))):
        with pytest.raises(ValueError, match="field='vector' needs the velocity components as columns"):
            StreamTracer(geom, z)
    for z in (np.zeros((n, 2)), np.zeros((n, 1)), np.zeros(n - 1)):
        with pytest.raises(ValueError, match="field='gradient' needs u"):
            StreamTracer(geom, z, field="gradient")
    with pytest.raises(ValueError, match="real numbers"):
        StreamTracer(geom, np.zeros((n, 2), dtype=complex))
    with pytest.raises(ValueError, match="real numbers"):
        StreamTracer(geom, np.full((n, 2), "a"))
    for field in ("flux", None, 0, "Vector"):
        with pytest.raises(ValueError, match="field must be 'vector' or 'gradient'"):
            StreamTracer(geom, np.zeros((n, 2)), field=field)


OK_KW = dict(step=0.1, max_steps=4)


@pytest.mark.parametrize("seeds,kw,match", [
    (np.zeros(2), OK_KW, r"seeds must be \(S, 2\)"),
    (np.zeros((3, 3)), OK_KW, r"seeds must be \(S, 2\)"),
    (np.zeros((3, 2, 1)), OK_KW, r"seeds must be \(S, 2\)"),
    (np.zeros((3, 2), dtype=complex), OK_KW, "seeds must be real numbers"),
    (np.full((3, 2), "a"), OK_KW, "seeds must be real numbers"),
    (np.zeros((3, 2)), dict(step=0.0, max_steps=4), "step must be finite and positive"),
    (np.zeros((3, 2)), dict(step=-0.1, max_steps=4), "step must be finite and positive"),
    (np.zeros((3, 2)), dict(step=np.nan, max_steps=4), "step must be finite and positive"),
    (np.zeros((3, 2)), dict(step=np.inf, max_steps=4), "step must be finite and positive"),
    (np.zeros((3, 2)), dict(step="x", max_steps=4), "must be numbers"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=0), "max_steps must be an integer >= 1"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=-3), "max_steps must be an integer >= 1"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=2.5), "max_steps must be an integer >= 1"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=True), "max_steps must be an integer >= 1"),
    (np.zeros((3, 2)), dict(OK_KW, min_speed=-1e-3), "min_speed must be finite and >= 0"),
    (np.zeros((3, 2)), dict(OK_KW, min_speed=np.nan), "min_speed must be finite and >= 0"),
    (np.zeros((3, 2)), dict(OK_KW, min_speed=np.inf), "min_speed must be finite and >= 0"),
    (np.zeros((3, 2)), dict(OK_KW, min_speed=None), "must be numbers"),
    (np.zeros((3, 2)), dict(OK_KW, direction="up"), "direction must be 'forward', 'backward' or 'both'"),
    (np.zeros((3, 2)), dict(OK_KW, direction=1), "direction must be 'forward', 'backward' or 'both'"),
    (np.zeros((3, 2)), dict(OK_KW, normalize=1), "normalize must be True or False"),
    (np.zeros((3, 2)), dict(OK_KW, normalize="yes"), "normalize must be True or False"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=2 ** 31 // 6), r"exceeds 32-bit indexing"),
    (np.zeros((3, 2)), dict(step=0.1, max_steps=2 ** 40), r"exceeds 32-bit indexing"),
    (np.broadcast_to(0.0, (2 ** 28, 2)), dict(step=0.1, max_steps=3), r"exceeds 32-bit indexing"),
])
def test_bad_trace_arguments_are_refused(no_library, seeds, kw, match):
    geom = m.fem2d(k=1)
    with pytest.raises(ValueError, match=match):
        streamlines(geom, np.zeros((_n(geom), 2)), seeds, **kw)
    with pytest.raises(ValueError, match=match):
        sl._check_trace(2, seeds, kw["step"], kw["max_steps"], kw.get("direction", "forward"),
                        kw.get("normalize", False), kw.get("min_speed", 0.0))


def test_the_count_just_below_the_limit_passes_the_check():
    P = np.broadcast_to(0.0, (2 ** 28 - 1, 2))
    sl._check_trace(2, np.zeros((1, 2)), 0.1, 2 ** 30 - 2, "forward", False, 0.0)       # 1 * (2^30 - 1) * 2 < 2^31
    with pytest.raises(ValueError, match="exceeds 32-bit indexing"):
        sl._check_trace(2, np.zeros((1, 2)), 0.1, 2 ** 30 - 1, "forward", False, 0.0)   # 1 * 2^30 * 2 = 2^31
    with pytest.raises(ValueError, match="exceeds 32-bit indexing"):
        sl._check_trace(2, P, 0.1, 4, "both", False, 0.0)


def test_streamlines_checks_the_field_before_device_work(no_library):
    geom = m.fem3d(k=1)
    with pytest.raises(ValueError, match="field='vector' needs"):
        streamlines(geom, np.zeros(_n(geom)), np.zeros((1, 3)), **OK_KW)
    with pytest.raises(ValueError, match="field='gradient' needs u"):
        streamlines(geom, np.zeros((_n(geom), 3)), np.zeros((1, 3)), field="gradient", **OK_KW)
    with pytest.raises(ValueError, match="field must be"):
        streamlines(geom, np.zeros((_n(geom), 3)), np.zeros((1, 3)), field="curl", **OK_KW)
