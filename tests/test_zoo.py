"""Zoo constructors on the host (no GPU): descriptors against the reference's definitions (src/Zoo/*.jl) and the
reference's smoke set (test/test_zoo.jl) solved by the oracle."""
import numpy as np
import pytest

import mgb_amd as m
from mgb_amd.convex import KIND_EP, KIND_LINEAR
from oracle import mgb_oracle as O


def _mg(dim):
    if dim == 1:
        return m.amg(m.fem1d(nodes=np.linspace(-1.0, 1.0, 5)))
    if dim == 2:
        return m.amg(m.fem2d_P1())
    return m.amg(m.fem3d(k=1))


def _D_names(prob):
    return list(prob.M[0].D_spec), list(prob.M[0].state_names)


def test_zoo_is_exported():
    for name in ("elastoplastic_torsion", "minimal_surface", "p_harmonic", "norton_hoff", "rof", "two_sided_obstacle"):
        assert callable(getattr(m.Zoo, name))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_elastoplastic_torsion_descriptor(dim):
    mg = _mg(dim)
    x = mg.geometry.xflat
    prob = m.Zoo.elastoplastic_torsion(mg, smax=1.5)
    nrows = dim + 2
    D_spec, states = _D_names(prob)
    assert states == ["u", "s"] and len(D_spec) == nrows
    fval = {1: 2.0, 2: 4.0, 3: 16.0}[dim]
    expect_f = np.zeros((x.shape[0], nrows)); expect_f[:, 0] = fval; expect_f[:, -1] = 0.5
    assert np.array_equal(prob.f, expect_f)
    assert np.array_equal(prob.g, np.tile([0.0, 1.5 ** 2 / 2], (x.shape[0], 1)))     # s_init = smax^2 / 2
    ep, lin = prob.Q.pieces
    assert ep.kind == KIND_EP and ep.idx == tuple(range(1, dim + 2)) and np.all(ep.p == 2.0)
    assert lin.kind == KIND_LINEAR and lin.idx == (nrows - 1,)
    assert np.all(lin.A == -1.0) and np.all(lin.b == 2.25)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_two_sided_obstacle_descriptor(dim):
    mg = _mg(dim)
    x = mg.geometry.xflat
    prob = m.Zoo.two_sided_obstacle(mg, psi_upper=lambda x: 0.5 + x[0])
    assert np.all(prob.f[:, 0] == {1: 1.0, 2: 2.0, 3: 8.0}[dim]) and np.all(prob.f[:, -1] == 0.5)
    assert np.all(prob.g[:, 1] == 10.0)
    ep, box = prob.Q.pieces
    assert ep.idx == tuple(range(1, dim + 2))
    assert box.kind == KIND_LINEAR and box.idx == (0,) and box.nc == 2
    assert np.array_equal(box.A, np.tile([1.0, -1.0], (x.shape[0], 1)))       # 2 x 1, column-major
    assert np.allclose(box.b[:, 0], 0.1) and np.array_equal(box.b[:, 1], 0.5 + x[:, 0])


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_rof_descriptor(dim):
    mg = _mg(dim)
    x = mg.geometry.xflat
    prob = m.Zoo.rof(mg, **{"λ": 3.0})
    nrows = dim + 3
    D_spec, states = _D_names(prob)
    assert states == ["u", "s", "r"] and len(D_spec) == nrows
    fd = 0.5 * np.tanh(5.0 * x[:, 0])
    assert np.array_equal(prob.g[:, 0], fd) and np.all(prob.g[:, 1:] == 10.0)       # g_u defaults to f_data
    assert np.all(prob.f[:, nrows - 2] == 1.0) and np.all(prob.f[:, nrows - 1] == 1.5)
    tv, data = prob.Q.pieces
    assert tv.idx == tuple(range(1, dim + 1)) + (nrows - 2,) and np.all(tv.p == 1.0)
    assert data.idx == (0, nrows - 1) and np.all(data.p == 2.0)
    assert np.array_equal(data.b[:, 0], -fd) and np.all(data.b[:, 1] == 0.0)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_minimal_surface_descriptor_and_shifted_cone(dim):
    mg = _mg(dim)
    x = mg.geometry.xflat
    prob = m.Zoo.minimal_surface(mg)
    g = (0.5 * x[:, 0] ** 2 if dim == 1 else 0.5 * (x[:, 0] ** 2 - x[:, 1] ** 2) if dim == 2 else 0.5 * np.sum(x ** 2, axis=1))
    assert np.allclose(prob.g[:, 0], g) and np.all(prob.g[:, 1] == 10.0)
    (pc,) = prob.Q.pieces
    nz = dim + 2
    assert pc.idx == tuple(range(nz)) and np.all(pc.p == 1.0)
    A = pc.A[0].reshape(nz, nz, order="F")
    rng = np.random.default_rng(1)
    for _ in range(5):
        grad, u, s = rng.standard_normal(dim), rng.standard_normal(), rng.standard_normal()
        y = np.concatenate([[u], grad, [s]])
        z = A @ y + pc.b[0]
        assert np.isclose(np.sum(z[:-1] ** 2), np.sum(grad ** 2) + 1.0) and z[-1] == s      # |q|^2 = |grad u|^2 + 1


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_p_harmonic_descriptor(dim):
    mg = _mg(dim)
    x = mg.geometry.xflat
    n = x.shape[0]
    prob = m.Zoo.p_harmonic(mg, p=1.7)
    nrows = dim * (dim + 1) + 1
    D_spec, states = _D_names(prob)
    assert states == [f"u{i}" for i in range(1, dim + 1)] + ["s"] and len(D_spec) == nrows
    assert D_spec[-1] == (dim, "id") and D_spec[dim + 1] == (1, "id")
    (pc,) = prob.Q.pieces
    expect_idx = tuple((i - 1) * (dim + 1) + j for i in range(1, dim + 1) for j in range(1, dim + 1)) + (nrows - 1,)
    assert pc.idx == expect_idx and pc.ni == dim * dim + 1 and np.all(pc.p == 1.7)
    assert np.array_equal(pc.A, np.tile(np.eye(pc.ni).reshape(1, -1), (n, 1)))
    f = np.zeros((n, nrows)); f[:, [i * (dim + 1) for i in range(dim)]] = 0.5; f[:, -1] = 1.0
    assert np.array_equal(prob.f, f)
    g1 = x[:, 0] ** 2 if dim == 1 else np.prod(x, axis=1)
    assert np.allclose(prob.g[:, 0], g1) and np.all(prob.g[:, 1:dim] == 0.0) and np.all(prob.g[:, dim] == 100.0)


def test_user_callables_are_called_once_per_node():
    mg = _mg(2)
    n = mg.geometry.xflat.shape[0]
    calls = []
    prob = m.Zoo.p_harmonic(mg, f=lambda x: (calls.append(1), (x[0], -x[1]))[1], g_u=lambda x: (x[1], 2.0))
    assert len(calls) == n
    assert np.array_equal(prob.f[:, 0], mg.geometry.xflat[:, 0]) and np.array_equal(prob.f[:, 3], -mg.geometry.xflat[:, 1])
    assert np.array_equal(prob.g[:, 0], mg.geometry.xflat[:, 1]) and np.all(prob.g[:, 1] == 2.0)


@pytest.mark.parametrize("dim", [2, 3])
def test_norton_hoff_packs_the_symmetric_gradient(dim):
    prob = m.Zoo.norton_hoff(_mg(dim))
    (pc,) = prob.Q.pieces
    nz = dim * dim + 1
    assert pc.ni == nz and np.all(pc.p == 1.5) and np.all(pc.b == 0.0)
    assert np.all(pc.A == pc.A[0])                                         # node-constant
    A = pc.A[0].reshape(nz, nz, order="F")
    rng = np.random.default_rng(2)
    for _ in range(5):
        Gr = rng.standard_normal((dim, dim))                               # Gr[i, j] = du_i / dx_j
        eps = 0.5 * (Gr + Gr.T)
        yidx = np.concatenate([Gr.reshape(-1), [rng.standard_normal()]])   # y[idx] = partials row-major by component, slack
        z = A @ yidx
        assert np.isclose(np.sum(z[:-1] ** 2), np.sum(eps ** 2)) and z[-1] == yidx[-1]
    off = 1.0 / np.sqrt(2.0)
    assert np.isclose(A[dim, 1], off) and np.isclose(A[dim, dim], off)     # (1, 2) pair: du1/dx2 and du2/dx1


def test_norton_hoff_raises_in_1d():
    with pytest.raises(ValueError, match="1D not supported"):
        m.Zoo.norton_hoff(_mg(1))


@pytest.mark.parametrize("name,dim", [("elastoplastic_torsion", 1), ("minimal_surface", 1), ("p_harmonic", 2),
                                      ("norton_hoff", 2), ("rof", 1), ("two_sided_obstacle", 1)])
def test_reference_smoke_set_solves_on_the_oracle(name, dim):
    """test/test_zoo.jl: fem1d with 3 nodes / fem2d_P1(), tol = 1e-3, finite z."""
    mg = m.amg(m.fem1d(nodes=np.linspace(-1.0, 1.0, 3))) if dim == 1 else m.amg(m.fem2d_P1())
    sol = O.mgb_solve(getattr(m.Zoo, name)(mg), tol=1e-3)
    assert np.all(np.isfinite(sol["z"]))
