"""StreamTracer / streamlines on the device against the NumPy twin (tests/streamlines_twin.py).

The twin takes its stage velocities from `interpolate()` at its own stage points (`gradient=True` for
`field="gradient"`), which is pinned elsewhere; the kernel evaluates by the same device functions, and every operation
after that is a fixed sequence of IEEE operations on both sides.  So `points`, `n` and `status` must be equal bit for bit,
NaN padding included, for every seed: there is no tolerance and no line is skipped.  The twin runs once per case on the
257 seeds; the 65 seeds are their first 65 (checked in tests/test_streamlines.py), and lines do not depend on each other.

The closed-form cases use the bound derived in tests/test_streamlines.py, `64 (n + 1) eps max(1, max|x|)` while
`P h <= 10` (`P` nodes per element).
"""
import ctypes as C

import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd.streamlines import StreamTracer, join_both, streamlines
from streamlines_twin import LEFT, MAX_STEPS, OUTSIDE, STALLED, join_twin, trace_twin
from test_streamlines import (EPS, GPU_CASES, GPU_MAX_STEPS, GPU_MIN_SPEED, GPU_STEP, LD, bound, gpu_seeds, scalar_field,
                              vector_field)

pytestmark = pytest.mark.gpu


def interpolated(geom, z, mode):
    """The twin's field: `interpolate()` at the twin's own stage points."""
    if mode == "vector":
        def v(P):
            vals, elem = m.interpolate(geom, z, P, return_element=True)
            return vals, elem >= 0
    else:
        def v(P):
            _, grads, elem = m.interpolate(geom, z, P, gradient=True, return_element=True)
            return grads, elem >= 0
    return v


def field_of(geom, mode):
    return vector_field(geom.xflat) if mode == "vector" else scalar_field(geom.xflat)


def same(a, b):
    return (np.array_equal(a.points, b.points, equal_nan=True) and np.array_equal(np.isnan(a.points), np.isnan(b.points))
            and np.array_equal(a.n, b.n) and np.array_equal(a.status, b.status))


@pytest.fixture(scope="module", params=[(c, f, nz) for c in sorted(GPU_CASES) for f in ("vector", "gradient")
                                        for nz in (False, True)], ids=lambda p: f"{p[0]}-{p[1]}-{'unit' if p[2] else 'raw'}")
def case(request):
    """One tracer per (mesh, field mode, normalize) with the twin's lines for the 257 seeds (computed once, read-only)."""
    name, mode, nz = request.param
    geom = GPU_CASES[name]()
    d = geom.xflat.shape[1]
    z = field_of(geom, mode)
    seeds = gpu_seeds(d, 257)
    twin = trace_twin(interpolated(geom, z, mode), seeds, GPU_STEP[nz], GPU_MAX_STEPS, normalize=nz,
                      min_speed=GPU_MIN_SPEED)
    for a in (twin.points, twin.n, twin.status):
        a.setflags(write=False)
    with StreamTracer(geom, z, field=mode) as st:
        yield name, mode, nz, geom, z, seeds, twin, st


@pytest.mark.parametrize("S", [65, 257])
def test_lines_are_bitwise_the_twins(case, S):
    name, mode, nz, geom, z, seeds, twin, st = case
    got = st.trace(seeds[:S], step=GPU_STEP[nz], max_steps=GPU_MAX_STEPS, normalize=nz, min_speed=GPU_MIN_SPEED)
    d = seeds.shape[1]
    assert got.points.shape == (S, GPU_MAX_STEPS + 1, d) and got.points.dtype == np.float64
    assert got.n.shape == got.status.shape == (S,) and got.n.dtype == got.status.dtype == np.int32
    counts = np.bincount(twin.status[:S], minlength=4)
    print(f"{name} {mode} normalize={nz} S={S}: MAX_STEPS/LEFT/STALLED/OUTSIDE = {list(counts)}")
    assert (counts > 0).all(), f"every status occurs on the twin: {list(counts)}"
    assert np.array_equal(got.n, twin.n[:S]), np.flatnonzero(got.n != twin.n[:S])
    assert np.array_equal(got.status, twin.status[:S]), np.flatnonzero(got.status != twin.status[:S])
    assert np.array_equal(np.isnan(got.points), np.isnan(twin.points[:S])), "the NaN padding matches in position"
    assert np.array_equal(got.points, twin.points[:S], equal_nan=True)
    # what the fields mean
    for i in range(S):
        assert np.isfinite(got.points[i, :got.n[i]]).all() and np.isnan(got.points[i, got.n[i]:]).all()
    assert np.array_equal(got.n == 0, got.status == OUTSIDE)
    assert np.array_equal(got.n == GPU_MAX_STEPS + 1, got.status == MAX_STEPS)
    inside = got.n > 0
    assert np.array_equal(got.points[inside, 0], seeds[:S][inside])


@pytest.mark.parametrize("name,mode", [("fem2d_k2", "vector"), ("fem2d_P1", "gradient"), ("fem3d_k1", "gradient")])
def test_reuse_and_determinism(name, mode):
    geom, nz = GPU_CASES[name](), False
    z, seeds = field_of(geom, mode), gpu_seeds(geom.xflat.shape[1], 65)
    with StreamTracer(geom, z, field=mode) as st:
        _reuse(st, geom, z, seeds, mode, nz)


def _reuse(st, geom, z, seeds, mode, nz):
    kw = dict(step=GPU_STEP[nz], max_steps=GPU_MAX_STEPS, normalize=nz, min_speed=GPU_MIN_SPEED)
    P = seeds[:65]
    a = st.trace(P, **kw)
    assert same(a, st.trace(P, **kw)), "two trace calls"
    assert same(a, streamlines(geom, z, P, field=mode, **kw)), "streamlines() is the class"
    back = st.trace(P, direction="backward", **kw)
    both = st.trace(P, direction="both", **kw)
    assert both.points.shape == (65, 2 * GPU_MAX_STEPS + 1, P.shape[1]) and both.status.shape == (65, 2)
    assert same(both, join_both(back, a)) and same(both, join_twin(back, a)), "both is the join of the two halves"
    perm = np.random.default_rng(7).permutation(65)
    b = st.trace(P[perm], **kw)
    assert np.array_equal(b.points, a.points[perm], equal_nan=True) and np.array_equal(b.n, a.n[perm])
    assert np.array_equal(b.status, a.status[perm]), "permuting the seeds permutes the result"
    # another field through set_field: a fresh tracer on it gives the same lines; -z forward is z backward
    z2 = -z
    with StreamTracer(geom, z2, field=mode) as fresh:
        c = fresh.trace(P, **kw)
    st.set_field(z2)
    try:
        assert same(c, st.trace(P, **kw)), "set_field equals a fresh tracer"
        assert same(c, back), "backward equals forward with -z"
    finally:
        st.set_field(z)
    assert same(a, st.trace(P, **kw))


# ---------------------------------------------------------------------------------------------------------------------
# closed forms on the device
# ---------------------------------------------------------------------------------------------------------------------

SEEDS2 = np.array([[0.3, -0.2], [-0.7, 0.45], [0.0, 0.9], [0.123456789, 0.25], [-0.5, -0.5], [0.5, 0.5], [0.0, 0.25]])


def _nodes_per_element(geom):
    return geom.x.shape[0]


@pytest.mark.parametrize("name", ["fem2d_k1", "fem2d_P1", "fem2d_k2", "fem2d_P2"])
def test_rotation_on_the_device(name):
    geom = GPU_CASES[name]()
    X = geom.xflat
    h, n = 0.05, 24
    assert _nodes_per_element(geom) * h <= 10
    got = streamlines(geom, np.stack([-X[:, 1], X[:, 0]], axis=1), SEEDS2, step=h, max_steps=n)
    assert np.array_equal(got.status, np.full(len(SEEDS2), MAX_STEPS))
    hl = LD(h)
    c, s = 1 - hl * hl / 2 + hl ** 4 / 24, hl - hl ** 3 / 6
    R = np.array([[c, -s], [s, c]], dtype=LD)
    want, worst = SEEDS2.astype(LD), 0.0
    for i in range(n + 1):
        err = float(np.abs(got.points[:, i].astype(LD) - want).max())
        worst = max(worst, err / bound(i, float(np.abs(want).max())))
        want = want @ R.T
    record_observation(f"streamlines rotation {name}: max error / bound {worst:.3e}")
    print(f"rotation {name}: max error / bound {worst:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["fem2d_k1", "fem2d_P2", "fem3d_k1", "fem3d_k2_curved"])
@pytest.mark.parametrize("normalize", [False, True])
def test_constant_field_on_the_device(name, normalize):
    geom = GPU_CASES[name]()
    d = geom.xflat.shape[1]
    c = np.array([0.6, -0.35, 0.2])[:d]
    h, n = 0.02, 24
    assert _nodes_per_element(geom) * h <= 10
    seeds = np.concatenate([SEEDS2, np.linspace(-0.4, 0.4, len(SEEDS2))[:, None]], axis=1)[:, :d] * 0.6
    got = streamlines(geom, np.tile(c, (geom.xflat.shape[0], 1)), seeds, step=h, max_steps=n, normalize=normalize)
    assert np.array_equal(got.status, np.full(len(seeds), MAX_STEPS))
    v = c / np.sqrt(np.sum(c * c)) if normalize else c
    worst = 0.0
    for i in range(n + 1):
        want = seeds + (i * h) * v
        worst = max(worst, np.abs(got.points[:, i] - want).max() / bound(i, np.abs(want).max()))
    record_observation(f"streamlines constant {name} normalize={normalize}: max error / bound {worst:.3e}")
    print(f"constant {name} normalize={normalize}: max error / bound {worst:.3e}")
    assert worst <= 1.0
    if normalize:
        chords = np.sqrt(np.sum(np.diff(got.points, axis=1) ** 2, axis=2))
        assert np.abs(chords - h).max() <= 64 * EPS


@pytest.mark.parametrize("make,label", [(lambda: GPU_CASES["fem2d_k2"](), "fem2d_k2"), (lambda: GPU_CASES["fem2d_P2"](), "fem2d_P2"),
                                        (lambda: m.fem3d(k=2), "fem3d_k2")])
def test_gradient_of_half_x_dot_x_on_the_device(make, label):
    geom = make()
    X = geom.xflat
    d = X.shape[1]
    h, n = 0.04, 24
    assert _nodes_per_element(geom) * h <= 10
    seeds = np.concatenate([SEEDS2, np.linspace(-0.4, 0.4, len(SEEDS2))[:, None]], axis=1)[:, :d] * 0.35
    got = streamlines(geom, 0.5 * np.sum(X * X, axis=1), seeds, step=h, max_steps=n, field="gradient")
    assert np.array_equal(got.status, np.full(len(seeds), MAX_STEPS))
    hl = LD(h)
    g = 1 + hl + hl * hl / 2 + hl ** 3 / 6 + hl ** 4 / 24
    want, worst = seeds.astype(LD), 0.0
    for i in range(n + 1):
        err = float(np.abs(got.points[:, i].astype(LD) - want).max())
        worst = max(worst, err / bound(i, float(np.abs(want).max())))
        want = want * g
    record_observation(f"streamlines quadratic {label}: max error / bound {worst:.3e}")
    print(f"quadratic {label}: max error / bound {worst:.3e}")
    assert worst <= 1.0


def test_zero_field_stalls_on_the_device():
    geom = GPU_CASES["fem2d_P1"]()
    got = streamlines(geom, np.zeros((geom.xflat.shape[0], 2)), SEEDS2, step=0.1, max_steps=5, normalize=True)
    assert np.array_equal(got.n, np.ones(len(SEEDS2))) and np.array_equal(got.status, np.full(len(SEEDS2), STALLED))
    assert np.array_equal(got.points[:, 0], SEEDS2) and np.isnan(got.points[:, 1:]).all()
    assert LEFT == 1


# ---------------------------------------------------------------------------------------------------------------------
# refusals through the C ABI
# ---------------------------------------------------------------------------------------------------------------------

def test_the_c_abi_refuses_the_count_and_a_closed_tracer_raises():
    from mgb_amd.device import ERR_INVALID
    geom = GPU_CASES["fem2d_k1"]()
    st = StreamTracer(geom, vector_field(geom.xflat))
    lib, dp, ip = st._ctx.lib, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    one, i1, i2 = np.zeros(4), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    args = (one.ctypes.data_as(dp), 0.1, 3, 0, 0.0, one.ctypes.data_as(dp), i1.ctypes.data_as(ip), i2.ctypes.data_as(ip))
    # S * (max_steps + 1) * d = 2^28 * 4 * 2 = 2^31: refused by count, nothing is read or allocated
    assert lib.mgbhip_stream_trace(st._handle, 2 ** 28, *args) == ERR_INVALID
    assert b"32-bit" in lib.mgbhip_last_error()
    big = (one.ctypes.data_as(dp), 0.1, 2 ** 31 - 2, 0, 0.0, one.ctypes.data_as(dp), i1.ctypes.data_as(ip), i2.ctypes.data_as(ip))
    assert lib.mgbhip_stream_trace(st._handle, 2, *big) == ERR_INVALID and b"32-bit" in lib.mgbhip_last_error()
    for bad in ((0.0, 3, 0, 0.0), (np.nan, 3, 0, 0.0), (0.1, 0, 0, 0.0), (0.1, 3, 0, -1.0), (0.1, 3, 0, np.nan)):
        a = (one.ctypes.data_as(dp),) + bad + (one.ctypes.data_as(dp), i1.ctypes.data_as(ip), i2.ctypes.data_as(ip))
        assert lib.mgbhip_stream_trace(st._handle, 1, *a) == ERR_INVALID, bad
    ok = st.trace(np.array([[0.5, 0.0]]), step=0.1, max_steps=3)
    assert ok.n[0] == 4
    st.close()
    st.close()
    with pytest.raises(ValueError, match="closed"):
        st.trace(np.array([[0.5, 0.0]]), step=0.1, max_steps=3)
    with pytest.raises(ValueError, match="closed"):
        st.set_field(vector_field(geom.xflat))
