"""The dense-operator kernels (csrc/dense.hip) at every tile, block and gate edge (DESIGN.md "Shape gates"): the hand-built
one-element problems of tests/dense_cases.py on the device.  Each test first asserts the path taken (p > 64 and N = 1: the dense
path; p = 64: the element kernels on the other side of the gate), then holds the result to the componentwise bound of
dense_cases.py.  The worst error / bound per case and kernel is recorded (helpers.record_observation); no assertion is tuned
from it."""
import numpy as np
import pytest

import dense_cases as D
from gate_cases import KERNEL_RTOL
from helpers import assert_z_close, record_observation

pytestmark = pytest.mark.gpu

_live = {}


@pytest.fixture(scope="module", autouse=True)
def _close_devices():
    yield
    for ctx, P in _live.values():
        P.close()
        ctx.close()
    _live.clear()


def device(name):
    from mgb_amd.device import DeviceProblem, HipContext
    if name not in _live:
        for ctx, P in _live.values():            # one resident problem at a time
            P.close()
            ctx.close()
        _live.clear()
        b = D.built(name)
        ctx = HipContext(0)
        P = DeviceProblem(ctx, b.M, b.Q)
        if b.bw is not None:
            P.set_barrier_weights(b.bw)
        _live[name] = (ctx, P)
    P = _live[name][1]
    if D.CASE[name].n > 64:
        assert P.p > 64 and P.N == 1, (name, P.p, P.N)
    else:
        assert P.p == 64 and P.N == 1, (name, P.p, P.N)
    return P


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _id(v):
    return v if isinstance(v, str) else str(v)


def _tag(name, level):
    return f"dense {name}/m{D.CASE[name].sizes[level]}"


@pytest.mark.parametrize("name,level", D.LEVELS, ids=_id)
def test_node_maps(name, level):
    """z0 + R s bit for bit, Dz rows within their bound (identity rows bit for bit), F and the slack against the oracle."""
    P = device(name)
    b = D.built(name)
    s, c, z0 = D.inputs(name, level)
    z_ref, dz = D.dz_reference(name, level)
    o = D.oracle_node(name, level)
    z = P.prolong_add(level, P.vec(s), P.vec(z0)).to_host()
    assert np.array_equal(z, z_ref)
    F, Dz = P.node_barrier(z, want_Dz=True)
    r = dz.ratios(Dz)
    record_observation(f"{_tag(name, level)} Dz: max error/bound {r.max():.3f}, skipped {dz.skipped:.3f}")
    assert r.max() <= 1.0, (name, level, r.max())
    n = b.case.n
    for k, (a, op) in enumerate(b.case.D_spec):
        if op == "id":
            assert np.array_equal(Dz[:, k], z_ref[a * n:(a + 1) * n]), (name, level, k)
    e_F, e_s = rel(F, o["F"]), rel(P.node_slack(z), o["slack"])
    record_observation(f"{_tag(name, level)} node_barrier / node_slack: relative error {e_F:.2e} / {e_s:.2e} (asserted 1e-12)")
    assert e_F <= 1e-12 and e_s <= 1e-12, (name, level, e_F, e_s)


@pytest.mark.parametrize("name,level", D.LEVELS, ids=_id)
def test_f0_and_f1(name, level):
    P = device(name)
    s, c, z0 = D.inputs(name, level)
    f0, _ = D.f0_reference(name, level)
    e0 = abs(P.f0(level, s, c, z0) - f0) / abs(f0)
    ref = D.f1_reference(name, level)
    r = ref.ratios(P.f1(level, s, c, z0))
    record_observation(f"{_tag(name, level)} f0: relative error {e0:.2e} (asserted {KERNEL_RTOL:.0e}); f1: max error/bound {r.max():.3e}, "
                       f"skipped {ref.skipped:.3f}")
    assert e0 <= KERNEL_RTOL, (name, level, e0)
    assert r.max() <= 1.0, (name, level, r.max())


@pytest.mark.parametrize("name,level", D.LEVELS, ids=_id)
def test_f2(name, level):
    P = device(name)
    s, c, z0 = D.inputs(name, level)
    ref = D.f2_reference(name, level)
    H = np.asarray(P.f2(level, s, c, z0).todense())
    m = H.shape[0]
    assert m == D.CASE[name].sizes[level]
    assert np.abs(H - H.T).max() <= 1e-13 * np.abs(H).max(), (name, level)          # symmetry, as test_gpu_gates._check_assembly
    r = ref.ratios(H)
    record_observation(f"{_tag(name, level)} f2: max error/bound {r.max():.3e}, skipped {ref.skipped:.3f}")
    worst = np.unravel_index(np.argmax(np.abs(H - ref.value) / np.where(ref.bound > 0, ref.bound, np.inf)), H.shape)
    assert r.max() <= 1.0, (name, level, r.max(), worst)                            # worst: (row, column) -> tile, K tail
    if D.CASE[name].n > 64:
        # the symmetric GEMM computes the tiles bi <= bj and stores each value twice: bitwise mirror across 64-tiles
        t = np.arange(m) // D.GT
        off = t[:, None] != t[None, :]
        assert np.array_equal(H[off], H.T[off]), (name, level)
    H2 = np.asarray(P.f2(level, s, c, z0).todense())
    assert np.array_equal(H, H2), (name, level)                                     # fixed summation order


def _solve_matches_oracle(prob, label, sizes):
    import mgb_amd as m
    from oracle import mgb_oracle as O
    assert [R.shape[1] for R in prob.M[0].R_fine] == sizes
    sol = m.mgb_solve(prob)
    so = O.mgb_solve(prob)
    assert_z_close(sol.z, so["z"], label)


def test_spectral2d_n17_solve_matches_oracle():
    """289 nodes: the first real geometry with a ragged second node block."""
    import mgb_amd as m
    _solve_matches_oracle(m.assemble(m.amg(m.spectral2d(n=17)), p=1.5), "spectral2d n=17 p=1.5 dense path", [4, 20, 100, 452, 514])


def test_spectral1d_n65_solve_matches_oracle():
    """65 nodes, the smallest dense size, with coarse levels on the 64-tile edges."""
    import mgb_amd as m
    _solve_matches_oracle(m.assemble(m.amg(m.spectral1d(n=65)), p=1.0), "spectral1d n=65 p=1.0 dense path", [2, 6, 14, 30, 62, 126, 128])
