"""Zoo problems on the device (-m gpu): the wide path (more than 10 D rows, power cones wider than four entries) and
the narrow one, primitive by primitive and end to end against the oracle, plus checks that do not lean on the oracle."""
import numpy as np
import pytest
import scipy.sparse as sp

import mgb_amd as m
from helpers import assert_z_close, stacked
from oracle import mgb_oracle as O

pytestmark = pytest.mark.gpu

KERNEL_RTOL = 1e-10


def rel(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _device(prob):
    from mgb_amd.device import DeviceMGBProblem
    return DeviceMGBProblem(prob)


def _check_primitives(P, Mo, Q, c, z0, rng, scale=1e-3, solve=True):
    """f0, f1, f2 and the solve on every level against the oracle (the pattern of test_gpu_parity.py)."""
    B = O.Barrier(Q)
    for J in range(len(Mo.R_fine)):
        R = Mo.R_fine[J]
        s = scale * rng.standard_normal(R.shape[1])
        y_o = B.f0(s, Mo.w, c, R, Mo.D_fine, z0)
        g_o = B.f1(s, Mo.w, c, R, Mo.D_fine, z0)
        H_o = sp.csr_matrix(B.f2(s, Mo.w, c, R, Mo.D_fine, z0))
        assert np.isfinite(y_o)
        assert abs(P.f0(J, s, c, z0) - y_o) <= KERNEL_RTOL * abs(y_o)
        g_d = P.f1(J, s, c, z0)
        assert rel(g_d, g_o) <= KERNEL_RTOL
        H_d = P.f2(J, s, c, z0)
        assert abs(H_d - H_o).max() <= KERNEL_RTOL * abs(H_o).max()
        assert abs(H_d - H_d.T).max() <= 1e-13 * abs(H_d).max()
        if solve:
            x_d = P.solve(J, g_d)
            x_o = O.solve_symmetric(sp.csc_matrix(H_o), g_o)
            assert rel(x_d, x_o) <= 1e-8
            assert np.linalg.norm(H_d @ x_d - g_d) <= 1e-9 * np.linalg.norm(g_d)


def _same_iteration_counts(a, b, finalize_slack=3):
    """Identical Newton counts on every t-step but the last (the finalize pass stops on a rounding-level rule)."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a[:, :-1], b[:, :-1])
    assert np.abs(a[:, -1] - b[:, -1]).max() <= finalize_slack


# Observed on an MI355X: 3-D two_sided_obstacle (narrow path) finalizes in 12 Newton steps against the oracle's 7 with z
# equal to 6.5e-15; every t-step before the finalize pass is identical.
FINALIZE_SLACK = {("two_sided_obstacle", "fem3d"): 6}


def _mg(kind):
    if kind == "fem1d":
        return m.amg(m.fem1d(nodes=np.linspace(-1.0, 1.0, 17)))
    if kind == "fem2d_P1":
        return m.amg(m.subdivide(m.fem2d_P1(), 3))
    if kind == "fem2d_P2":
        return m.amg(m.subdivide(m.fem2d_P2(), 2))
    if kind == "fem3d":
        return m.amg(m.subdivide(m.fem3d(k=1), 2))
    if kind == "spectral2d":
        return m.amg(m.spectral2d(n=9))
    raise ValueError(kind)


@pytest.mark.parametrize("name,kind", [("p_harmonic", "fem2d_P1"), ("p_harmonic", "fem2d_P2"), ("p_harmonic", "fem3d"),
                                       ("norton_hoff", "fem2d_P1"), ("norton_hoff", "fem2d_P2"), ("norton_hoff", "fem3d"),
                                       ("minimal_surface", "fem3d")])
def test_wide_primitives_match_oracle(name, kind):
    prob = getattr(m.Zoo, name)(_mg(kind))
    D = _device(prob)
    try:
        _check_primitives(D.main, O.OracleAMG(prob.M[0]), prob.Q, 0.1 * prob.f, stacked(prob.g), np.random.default_rng(11),
                          scale=1e-3)
    finally:
        D.close()


def test_wide_phase1_cobarrier_primitives_match_oracle():
    """Phase-I image of 2-D p_harmonic: 7 + 1 + 3 = 11 D rows, nu = 4, cobarrier of a 5-wide cone plus the box terms."""
    prob = m.Zoo.p_harmonic(_mg("fem2d_P1"))
    n = prob.M[0].w.size
    nD = len(prob.M[0].D_fine)
    assert len(prob.M[1].D_fine) == 11
    D = _device(prob)
    try:
        feas = D.feasibility
        feas.set_box(300.0, 400.0)
        Qf = O.FeasConvex(prob.Q, 300.0, 400.0, nD + 1)
        z1 = np.concatenate([stacked(prob.g), np.full(n, 3.0)])
        c1 = np.zeros((n, nD + 1 + 3)); c1[:, nD] = 1.0
        _check_primitives(feas, O.OracleAMG(prob.M[1]), Qf, c1, z1, np.random.default_rng(5), scale=1e-4)
    finally:
        D.close()


E2E = [(name, kind) for name in ("elastoplastic_torsion", "minimal_surface", "p_harmonic", "rof", "two_sided_obstacle")
       for kind in ("fem1d", "fem2d_P1", "fem3d")] + [("norton_hoff", "fem2d_P1"), ("norton_hoff", "fem3d"),
                                                      ("p_harmonic", "spectral2d")]


@pytest.mark.parametrize("name,kind", E2E)
def test_zoo_solve_matches_oracle(name, kind):
    prob = getattr(m.Zoo, name)(_mg(kind))
    sol = m.mgb_solve(prob)
    ref = O.mgb_solve(prob)
    assert (sol.SOL_feasibility is None) == (ref["SOL_feasibility"] is None)
    assert_z_close(sol.z, ref["z"], f"zoo {name} {kind}")
    _same_iteration_counts(sol.SOL_main["its"], ref["SOL_main"]["its"], FINALIZE_SLACK.get((name, kind), 3))


def test_p_harmonic_phase1_matches_oracle():
    """A small s_init makes the start infeasible (s < |grad u|^p): phase I runs on the wide path (11 D rows, nu = 4)."""
    prob = m.Zoo.p_harmonic(_mg("fem2d_P1"), s_init=0.01)
    sol = m.mgb_solve(prob)
    ref = O.mgb_solve(prob)
    assert sol.SOL_feasibility is not None and ref["SOL_feasibility"] is not None
    assert_z_close(sol.z, ref["z"], "zoo p_harmonic phase I")
    _same_iteration_counts(sol.SOL_main["its"], ref["SOL_main"]["its"])


def test_minimal_surface_reproduces_affine_boundary_data():
    """On P1 an affine trace is the minimal surface; the solve returns it to solver tolerance."""
    mg = _mg("fem2d_P1")
    sol = m.mgb_solve(m.Zoo.minimal_surface(mg, g_u=lambda x: 0.3 * x[0] - 0.2 * x[1] + 0.1))
    x = mg.geometry.xflat
    assert np.abs(sol.z[:, 0] - (0.3 * x[:, 0] - 0.2 * x[:, 1] + 0.1)).max() <= 1e-6


def test_elastoplastic_torsion_respects_the_yield_bound():
    mg = _mg("fem2d_P1")
    sol = m.mgb_solve(m.Zoo.elastoplastic_torsion(mg))
    prob = m.Zoo.elastoplastic_torsion(mg)
    y = O.apply_D(O.OracleAMG(prob.M[0]).D_fine, stacked(sol.z))      # rows: u, du/dx, du/dy, s at every node
    gx, gy = y[:, 1], y[:, 2]
    assert np.sqrt(gx ** 2 + gy ** 2).max() <= 1.0 + 1e-6
    assert np.sqrt(gx ** 2 + gy ** 2).max() >= 0.9            # the bound is active somewhere (default forcing)


def test_two_sided_obstacle_stays_between_the_obstacles():
    sol = m.mgb_solve(m.Zoo.two_sided_obstacle(_mg("fem2d_P1")))
    u = sol.z[:, 0]
    assert u.min() >= -0.1 - 1e-9 and u.max() <= 1.0 + 1e-9
    assert u.min() <= -0.09                                    # the lower obstacle is reached (default forcing)


def test_p_harmonic_at_p2_decouples_into_the_scalar_problem():
    """p = 2, f = (0.5, 0), g_u = (x^2 + y^2, 0): u2 = 0 and u1 is the scalar default problem assemble(mg, p=2).
    Both solves see the same Newton systems up to the decoupled zero block of u2: observed on an MI355X, max|u1 - u| = 0
    and max|u2| = 0 exactly (fem2d_P1, L = 3).  Asserted with margin at 1e-10 (and recorded in parity_observed.txt)."""
    mg = _mg("fem2d_P1")
    vec = m.mgb_solve(m.Zoo.p_harmonic(mg, p=2.0, f=lambda x: (0.5, 0.0), g_u=lambda x: (x[0] ** 2 + x[1] ** 2, 0.0)))
    sca = m.mgb_solve(m.assemble(mg, p=2.0))
    from helpers import record_observation
    d1 = float(np.abs(vec.z[:, 0] - sca.z[:, 0]).max())
    record_observation(f"zoo p_harmonic p=2 vs scalar: max|u1 - u| {d1:.2e}, max|u2| {np.abs(vec.z[:, 1]).max():.2e}")
    assert np.abs(vec.z[:, 1]).max() <= 1e-10
    assert d1 <= 1e-10


def test_3d_vector_phase1_raises_the_state_limit_then_solves():
    mg = _mg("fem3d")
    with pytest.raises(ValueError, match="MAX_NU"):
        m.mgb_solve(m.Zoo.p_harmonic(mg, s_init=0.01))
    sol = m.mgb_solve(m.Zoo.p_harmonic(mg))
    assert sol.SOL_feasibility is None and np.all(np.isfinite(sol.z))
