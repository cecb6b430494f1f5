"""ResidualEstimator on the device against the 50-digit evaluation of the same formulas (tests/residual_twin.py `Exact`,
with tests/faces_twin.py for the jumps), at every shape the launch plan branches on, for the zero cases and for the order
guarantees.

The bound.  Every comparison with the exact value is `|device - exact| <= c eps A`, eps = 2^-52.  `A` is what `Exact`
returns next to the value.  For the strong residual r = f + div a it is `fabs + (1 + |p-2|) G |(J^T J)^-1|_F Mm`: r is a
sum that may cancel (it vanishes for an exact solution), so it is measured against `fabs = sum_i |phi_i f_i|` (`|f_q|` for
a source given at the points) and the absolute terms of div a, never against |r|.  `Mm = |sum_i |d2phi_i| |z_i||_F +
T (sum_a |sum_i |d2phi_i| |x_i,a||_F^2)^(1/2)` bounds `M = H_xi(z) - sum_a g_a H_xi(x_a)` and what its roundings are
proportional to, `T = |J^-1|_2 (|J|abs,F |g| + |sum_i |dphi_i| |z_i||_2) >= |g|` does the same for g = grad u, `G` is
the power `|g|^(p-2)` at the worst gradient within 1e-3 T of g, and `tr H = sum M_bc (J^T J)^-1_bc` and
`g^T H g / |g|^2 = v^T M v / |g|^2`, `v = J^-1 g`, are both at most `|(J^T J)^-1|_F |M|_F`: J^-1 enters twice, so cond(J)
enters squared, through `|(J^T J)^-1|_F` in A and through the constants below.  The interior value is measured against
`h_K^2 sum_q measure_q A_q^2`: (r + dr)^2 - r^2 = 2 r dr and |r| <= A.

`c` is counted from the kernel's operations, to first order, in units of the unit roundoff u = eps / 2.  With n the nodes
of an element, D the dimension, Ms = D (D + 1) / 2, c_cof = 0, 3 the roundings of a cofactor and c_det = 3, 5 those of the
determinant behind it for D = 2, 3 (csrc/residual.hip forms both without contraction), and three numbers of the mesh,
the tables and the data: kJ = max |J^-1|_2 |J|abs,F, k = max cond_2(J) and rho = max T / |g| (`Exact.kJ`, `.kappa`, `.rho`),

  e_cf  = c_cof k^2 + (c_det + c_cof) k + 1      J^-1 = C^T / det J beyond the rounding of J: cofactors (|J|^2 <= k |C|),
                                                 determinant (|J| |C| / det = k), reciprocal
  E_g   = n + e_cf + (D + 1) k                   grad u against T: the chains of J and xi (n, inside T), the closed form, the
                                                 products C xi / det (D + 1 roundings of terms <= k |g|)
  E_M   = n + D + E_g                            M against Mm: the chains of H_xi(z) and H_xi(x_a), the D fused subtractions,
                                                 the error of g times |H_xi(x_a)|
  E_Gi  = 2 sqrt(D) (n kJ + e_cf) + D + 2        (J^T J)^-1 = J^-1 J^-T in the Frobenius norm: twice the relative error of
                                                 J^-1, |J^-1|_F |J^-1|_2 <= sqrt(D) |(J^T J)^-1|_F; its chain and two products
  E_tr  = E_M + E_Gi + Ms                        tr H against |(J^T J)^-1|_F Mm: the chain over the Ms entries
  p = 2:   C_r = E_tr + 1                        the addition of f (its own chain, n, is below E_tr)
  E_v   = n kJ + e_cf + D + 1 + E_g rho          v = C^T g / det against |J^-1|_2 |g|: the relative error of g is E_g rho
  E_q   = 2 E_v + 2 E_g rho + E_M + Ms + D + 3   v^T M v / |g|^2: v twice, |g|^2 (the error of g, its D roundings), M, the
                                                 products and the chain, the division
  E_G   = |p - 2| (E_g rho + D / 2) + 5          |g|^(p-2) through |g|^2; pow to 2 ulp and its exponent (p = 1: a root and a
                                                 division, below that)
  p != 2:  C_r = max(E_tr, E_q + 1) + 1 + E_G + 2        ... the product with p - 2 and the sum; the product with the power;
                                                 the addition of f
  E_meas = D n kJ + (c_det + c_cof) k^(D-1) + 1  det J moves by tr(J^-1 dJ); the closed form; times w_q
  C_int = 2 C_r + E_meas + 2                     r^2 and the product with the measure
          + 2 ((E_meas + Q - 1) / D + 4) + 2     h_K^2: |K| is a sum of Q measures, the root (cbrt to 2 ulp), h_K h_K, the product

and the sums add `L = ceil(log2 S) + ceil(Q / S) - 1` roundings per element and 2 for the compensated reduction:

  strong residual  c = 1.05 C_r / 2,      interior  c = 1.05 (C_int + L + 2) / 2,

5 % for the terms of second order; C u < 1e-3 is asserted, which is also what the 1e-3 T in G needs.  The jump half of
`estimate` is `Faces.indicator`: the jumps within the `jflux` constant of tests/test_gpu_faces.py, the face sizes (a sum
of Qf measures, each within E_ds, which that constant contains), the product and the gather over F faces:
c_ind = 2 c_jflux + 1.05 (Qf + F + 3) / 2; the sum of the two halves on the host adds one rounding.

Nothing in c comes from an observed error.  The largest observed error / bound per family is printed by the tests and
recorded in DESIGN.md section 8.
"""
import ctypes as C
import dataclasses
import math
import sys

import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.estimate  # noqa: F401
import mgb_amd.faces  # noqa: F401
import mgb_amd.integrate  # noqa: F401
import faces_twin
import residual_twin as RT
import test_gpu_faces as TF
from integrate_twin import Twin

pytestmark = pytest.mark.gpu

E = sys.modules["mgb_amd.estimate"]
Fm = sys.modules["mgb_amd.faces"]
I = sys.modules["mgb_amd.integrate"]
EPS = float(np.finfo(np.float64).eps)
PS = (1.0, 1.5, 2.0, 4.0)


def constants(ex, p):
    """(C_r, C_int + L + 2) in units of u for an `Exact` whose `fields` have seen the data of the comparison."""
    n, D, Q = ex.p, ex.d, ex.Q
    kJ, k, rho = ex.kJ, ex.kappa, ex.rho
    Ms = D * (D + 1) // 2
    c_cof, c_det = (0, 3) if D == 2 else (3, 5)
    e_cf = c_cof * k ** 2 + (c_det + c_cof) * k + 1
    e_g = n + e_cf + (D + 1) * k
    e_m = n + D + e_g
    e_gi = 2 * math.sqrt(D) * (n * kJ + e_cf) + D + 2
    e_tr = e_m + e_gi + Ms
    if p == 2.0:
        c_r = e_tr + 1
    else:
        e_v = n * kJ + e_cf + D + 1 + e_g * rho
        e_q = 2 * e_v + 2 * e_g * rho + e_m + Ms + D + 3
        e_G = abs(p - 2.0) * (e_g * rho + D / 2) + 5
        c_r = max(e_tr, e_q + 1) + 1 + e_G + 2
    e_meas = D * n * kJ + (c_det + c_cof) * k ** (D - 1) + 1
    c_int = 2 * c_r + e_meas + 2 + 2 * ((e_meas + Q - 1) / D + 4) + 2
    S = min(Q, 256)
    L = math.ceil(math.log2(S)) + math.ceil(Q / S) - 1 if S > 1 else 0
    assert c_int * EPS / 2 < 1e-3
    return c_r, c_int + L + 2


def c_pointwise(ex, p):
    return 1.05 * constants(ex, p)[0] / 2


def c_interior(ex, p):
    return 1.05 * constants(ex, p)[1] / 2


def c_indicator(fex, p, F):
    return 2 * TF.bound_constant("jflux", p, fex) + 1.05 * (fex.Qf + F + 3) / 2


# ---- the cases, built once --------------------------------------------------------------------------------------------

_CACHE = {}


def setup(name, geom=None, order=None, ncol=2, faces=True):
    """The geometry, the tables, the exact evaluators, the data (Z, the source in both forms) and the exact fields of a
    case, built once and left unchanged."""
    key = (name, order, ncol)
    if key not in _CACHE:
        if geom is None:
            mk, order = RT.cases(m)[name]
            geom = mk()
        x, tb = RT.tables(geom, order)
        ex = RT.Exact(x, tb)
        Z, F = RT.data(geom, ncol)
        Fq = RT.source_at(np.einsum("qi,ina->nqa", tb["phi"], x))
        fld = ex.fields(Z, F)
        S = dict(geom=geom, order=order, tb=tb, ex=ex, Z=Z, F=F, Fq=Fq, fld={1: fld, 2: dict(fld, **ex.source(Fq))}, res={})
        if faces:
            ftb = Fm.face_tables(geom)
            _, itr, ori, ef = faces_twin.topology(geom.t, ftb["corners"])
            S.update(fex=faces_twin.Exact(geom.x, ftb), itr=itr, ori=ori, ef=ef, fcache={}, ind={})
        _CACHE[key] = S
    return _CACHE[key]


def exact_interior(S, form, p):
    if (form, p) not in S["res"]:
        ex = S["ex"]
        S["res"][form, p] = (ex.residual(S["fld"][form], p), ex.interior(S["fld"][form], p))
    return S["res"][form, p]


def exact_indicator(S, p):
    if p not in S["ind"]:
        S["ind"][p] = RT.indicator(S["fex"], S["itr"], S["ori"], S["ef"], S["Z"], p, cache=S["fcache"])
    return S["ind"][p]


def _within(label, dev, exact, A, c, ratios):
    err, bound = abs(float(exact - float(dev))), c * EPS * A
    ratios.append(err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
    assert err <= bound, (label, err, bound, float(dev), float(exact))


def check_element_residual(S, est, form, p, label, ratios):
    """strong_residual and interior of every column against the exact values; returns the device's interior values."""
    ex, Z = S["ex"], S["Z"]
    src = S["F"] if form == 1 else S["Fq"]
    (r, A), (vals, As, tot, Atot) = exact_interior(S, form, p)
    cp, ci = c_pointwise(ex, p), c_interior(ex, p)
    dev_r = est.strong_residual(Z, src, p=p)
    dev_v, dev_t = est.interior(Z, src, p=p)
    ncol = Z.shape[1]
    assert dev_r.shape == (ex.N, ex.Q, ncol) and dev_v.shape == (ex.N, ncol) and dev_t.shape == (ncol,)
    rr, ri = [], []
    for c in range(ncol):
        for n in range(ex.N):
            for q in range(ex.Q):
                _within((label, form, p, "r", n, q, c), dev_r[n, q, c], r[n, q, c], A[n, q, c], cp, rr)
            _within((label, form, p, "interior", n, c), dev_v[n, c], vals[c][n], As[c][n], ci, ri)
        _within((label, form, p, "total", c), dev_t[c], tot[c], Atot[c], ci, ri)
    print(f"{label} source form {form} p={p}: largest error / bound: strong residual {max(rr):.3e}, interior {max(ri):.3e}")
    ratios += rr + ri
    return dev_v


# ---- 1. device against the 50-digit twin: every family, p and both forms of the source ---------------------------

@pytest.mark.parametrize("name", sorted(RT.cases(m)))
def test_device_against_the_exact_values(name):
    S = setup(name)
    ex, Z = S["ex"], S["Z"]
    assert RT.gradient_norms(S["geom"].x, S["tb"], Z).min() > 0.5
    ratios = []
    with m.ResidualEstimator(S["geom"], order=S["order"]) as est:
        assert est.n_points == ex.Q and est.n_elements == ex.N
        h = est.element_sizes()
        for n, hk in enumerate(ex.sizes()):
            assert abs(float(hk - float(h[n]))) <= c_interior(ex, 2.0) * EPS * float(hk)
        for p in PS:
            for form in (1, 2):
                dev_v = check_element_residual(S, est, form, p, name, ratios)
            # estimate: the sum of the two halves, the source at the points
            eta2, total = est.estimate(Z, S["Fq"], p=p)
            jump, _ = est.faces.indicator(Z, p)
            assert np.array_equal(eta2, dev_v + jump)
            assert np.array_equal(total, [math.fsum(eta2[:, c]) for c in range(Z.shape[1])])
            (_, _), (vals, As, _, _) = exact_interior(S, 2, p)
            ind, Aind = exact_indicator(S, p)
            ci, cj = c_interior(ex, p), c_indicator(S["fex"], p, est.faces.n_local_faces)
            for c in range(Z.shape[1]):
                bounds = [EPS * (ci * As[c][n] + cj * Aind[c][n] + 0.5 * (As[c][n] + Aind[c][n])) for n in range(ex.N)]
                for n in range(ex.N):
                    err = abs(float(vals[c][n] + ind[c][n] - float(eta2[n, c])))
                    ratios.append(err / bounds[n])
                    assert err <= bounds[n], (name, p, "eta2", n, c, err, bounds[n])
                exact_total = RT.MP.fsum(vals[c]) + RT.MP.fsum(ind[c])
                bt = sum(bounds) + 0.5 * EPS * abs(float(exact_total))
                assert abs(float(exact_total - float(total[c]))) <= bt, (name, p, "total", c)
    print(f"RATIO {name}: largest error / bound = {max(ratios):.3e}")


# ---- 2. zero tests, end to end ---------------------------------------------------------------------------------------

AFFINE = {
    "fem2d_k2": lambda: m.fem2d(k=2, K=m.subdivide(m.fem2d(k=2), 2).x @ np.array([[1.0, -0.2], [0.35, 0.8]])),
    "fem2d_k3": lambda: m.fem2d(k=3, K=m.subdivide(m.fem2d(k=3), 2).x @ np.array([[1.0, -0.2], [0.35, 0.8]])),
    "fem2d_P2": lambda: m.fem2d_P2(K=m.subdivide(m.fem2d_P2(), 2).x @ np.array([[1.0, -0.2], [0.35, 0.8]])),
    "fem2d_P2_nobubble": lambda: m.fem2d_P2(bubble=False,
                                            K=m.subdivide(m.fem2d_P2(bubble=False), 2).x @ np.array([[1.0, -0.2], [0.35, 0.8]])),
}


@pytest.mark.parametrize("name", sorted(AFFINE))
def test_an_exact_quadratic_solution_has_a_zero_estimate(name):
    """u = x^2 - 0.5 x y + 2 y^2 lies in the element space on an affine mesh, -lap u = -6: with f = -6 at the points the
    interior residual and the flux jumps are both rounding, each within its own bound of zero."""
    geom = AFFINE[name]()
    x, tb = RT.tables(geom)
    X = geom.xflat
    z = X[:, 0] ** 2 - 0.5 * X[:, 0] * X[:, 1] + 2.0 * X[:, 1] ** 2
    ex = RT.Exact(x, tb)
    f = np.full((ex.N, ex.Q), -6.0)
    fld = ex.fields(z, f)
    vals, As, tot, Atot = ex.interior(fld, 2.0)
    ftb = Fm.face_tables(geom)
    _, itr, ori, ef = faces_twin.topology(geom.t, ftb["corners"])
    fex = faces_twin.Exact(geom.x, ftb)
    ind, Aind = RT.indicator(fex, itr, ori, ef, z, 2.0)
    with m.ResidualEstimator(geom) as est:
        r = est.strong_residual(z, f)
        (rx, A) = ex.residual(fld, 2.0)
        cp = c_pointwise(ex, 2.0)
        for n in range(ex.N):
            for q in range(ex.Q):
                assert abs(r[n, q] - float(rx[n, q, 0])) <= cp * EPS * A[n, q, 0]
        eta2, total = est.estimate(z, f)
        ci, cj = c_interior(ex, 2.0), c_indicator(fex, 2.0, est.faces.n_local_faces)
        bound = EPS * ((ci + 0.5) * Atot[0] + (cj + 0.5) * math.fsum(Aind[0]))
        exact_total = float(tot[0] + RT.MP.fsum(ind[0]))
        print(f"{name}: estimate total {total:.3e}, exact {exact_total:.3e}, bound {bound:.3e}; sum of f^2 h^2 |K| = "
              f"{36.0 * float(np.sum(est.element_sizes() ** 2 * est.weights().sum(axis=1))):.3e}")
        assert abs(total - exact_total) <= bound and 0.0 <= total <= exact_total + bound
        assert exact_total <= bound                  # the exact value of the discrete sums is itself rounding of z and the tables


@pytest.mark.parametrize("p", PS)
def test_p1_strong_residual_is_the_source_bit_for_bit(p):
    """The second-derivative tables of fem2d_P1 are zero, so every term of div a vanishes exactly and r = f + 0."""
    S = setup("fem2d_P1")
    with m.ResidualEstimator(S["geom"]) as est:
        r = est.strong_residual(S["Z"], S["Fq"], p=p)
        for c in range(S["Z"].shape[1]):
            assert np.array_equal(r[:, :, c], S["Fq"])
        tw = Twin(np.asarray(S["geom"].x), S["tb"])
        fq = tw.u_fused(S["F"])[:, :, 0]             # the chain of fused multiply-adds the device carries f to the points with
        r = est.strong_residual(S["Z"], S["F"], p=p)
        for c in range(S["Z"].shape[1]):
            assert np.array_equal(r[:, :, c], fq)
        zc = np.full(S["Z"].shape[0], 3.0)           # grad u = 0: div a = 0 by convention for p != 2, and tr H = 0 for p = 2
        assert np.array_equal(est.strong_residual(zc, S["Fq"], p=p), S["Fq"])


# ---- 3. shape edges: every size the plan branches on ---------------------------------------------------------------

def _edge(label, geom, order, ncol=1, p=1.5):
    S = setup(label, geom=geom, order=order, ncol=ncol, faces=False)
    ratios = []
    with m.ResidualEstimator(geom, order=order) as est:
        pl = est.plan()
        for form in (1, 2):
            check_element_residual(S, est, form, p, label, ratios)
        check_element_residual(S, est, 2, 2.0, label, ratios)
    print(f"RATIO {label}: largest error / bound = {max(ratios):.3e}; plan {pl}")
    return pl


def test_edge_last_group_is_a_tail():
    full = m.subdivide(m.fem2d(k=2), 4)
    G = E.plan(2, 9, 16, 1)["G"]
    assert G > 1 and full.x.shape[1] >= G + 1
    geom = m.fem2d(k=2, K=RT.warp(full.x)[:, :G + 1, :])
    pl = _edge("tail", geom, 4)
    assert pl["S"] == 16 and pl["G"] == G == 16 and pl["groups"] == 2 and geom.x.shape[1] == G + 1


def test_edge_lanes_take_two_points():
    geom = m.fem3d(k=1, K=RT.warp(m.subdivide(m.fem3d(k=1), 2).x, 0.03)[:, :2, :])
    pl = _edge("Q343", geom, 7)
    assert pl["S"] == pl["threads"] == 256 and 7 ** 3 > pl["S"]


@pytest.mark.parametrize("order", [4, 5])
def test_edge_largest_staged_and_first_unstaged_tables(order):
    geom = m.fem3d(k=2, K=RT.warp(m.subdivide(m.fem3d(k=2), 2).x, 0.03)[:, :2, :])
    pl = _edge(f"tables_order{order}", geom, order)
    qp = I.plan(3, 3, 27, order ** 3, 2)
    assert (pl["S"], pl["G"]) == (qp["S"], qp["G"]) and pl["lds"] - pl["tables_lds"] * pl["table_bytes"] == \
        qp["lds"] - qp["tables_lds"] * qp["table_bytes"]                      # the base is Quadrature's
    assert pl["tables_lds"] == (1 if order == 4 else 0) and qp["tables_lds"] == 1
    assert pl["table_bytes"] == (138240 if order == 4 else 270000)


def test_edge_more_columns_than_a_chunk():
    mk, order = RT.cases(m)["fem2d_k1"]
    pl = _edge("ncol5", mk(), order, ncol=5)
    assert pl["chunk"] == 4


# ---- 4. order guarantees, bitwise ------------------------------------------------------------------------------------

def test_a_column_does_not_depend_on_its_company():
    S = setup("fem2d_P2", ncol=5)
    Z = S["Z"]
    with m.ResidualEstimator(S["geom"]) as est:
        assert Z.shape[1] == est.plan()["chunk"] + 1
        for p in (1.5, 2.0):
            for src in (S["F"], S["Fq"]):
                r, (v, t), (e, et) = est.strong_residual(Z, src, p=p), est.interior(Z, src, p=p), est.estimate(Z, src, p=p)
                v2, t2 = est.interior(Z, src, p=p)
                assert np.array_equal(v, v2) and np.array_equal(t, t2)                          # run to run
                for c in range(Z.shape[1]):
                    vc, tc = est.interior(Z[:, c], src, p=p)
                    ec, etc = est.estimate(Z[:, c], src, p=p)
                    assert isinstance(tc, float) and tc == t[c] and np.array_equal(vc, v[:, c])
                    assert isinstance(etc, float) and etc == et[c] and np.array_equal(ec, e[:, c])
                    assert np.array_equal(est.strong_residual(Z[:, c], src, p=p), r[:, :, c])
        # the total with and without the element values (the C entry takes NULL for them)
        from mgb_amd.device import _check, _ptr
        Zc, Fc, tot = np.ascontiguousarray(Z), np.ascontiguousarray(S["F"]), np.empty(Z.shape[1])
        _check(est._ctx.lib, est._ctx.lib.mgbhip_residual_integrate(est._handle, C.c_double(1.5), Z.shape[1], _ptr(Zc), _ptr(Fc), 0,
                                                                    None, _ptr(tot)))
        assert np.array_equal(tot, est.interior(Z, S["F"], p=1.5)[1])


def test_an_element_does_not_depend_on_the_rest_of_the_mesh():
    full = RT.warp(m.subdivide(m.fem2d(k=2), 4).x)
    G = E.plan(2, 9, 16, 1)["G"]
    big = m.fem2d(k=2, K=full[:, :2 * G + 1, :])
    part = m.fem2d(k=2, K=full[:, G:2 * G, :])                                  # the second group, as a mesh of its own
    Zb, Fb = RT.data(big)
    Zp, Fp = RT.data(part)
    nodes = slice(9 * G, 18 * G)
    assert np.array_equal(Zb[nodes], Zp) and np.array_equal(Fb[nodes], Fp)
    with m.ResidualEstimator(big, order=4) as eb, m.ResidualEstimator(part, order=4) as ep:
        assert eb.plan()["G"] == G and eb.plan()["groups"] == 3 and ep.plan()["groups"] == 1
        for p in (1.5, 2.0):
            vb, _ = eb.interior(Zb, Fb, p=p)
            vp, _ = ep.interior(Zp, Fp, p=p)
            assert np.array_equal(vb[G:2 * G], vp)
            assert np.array_equal(eb.strong_residual(Zb, Fb, p=p)[G:2 * G], ep.strong_residual(Zp, Fp, p=p))
        assert np.array_equal(eb.element_sizes()[G:2 * G], ep.element_sizes())
        assert np.array_equal(eb.weights()[G:2 * G], ep.weights())


@pytest.mark.parametrize("name", sorted(RT.cases(m)))
def test_one_shot_functions_and_the_untouched_entries(name):
    """The one-shot functions return the object's bits; and next to a ResidualEstimator, Faces.indicator, jump_indicator
    and Quadrature.integrate return what they return on their own."""
    S = setup(name)
    geom, order, Z, F = S["geom"], S["order"], S["Z"], S["F"]
    with m.Quadrature(geom, order=order) as q:
        w1p_before = q.integrate(Z, kind="w1p", p=1.5, per_element=True)
        energy_before = q.integrate(Z, kind="energy", p=1.5, source=F)
    with m.Faces(geom) as fc:
        ind_alone = fc.indicator(Z, p=1.5)
    with m.ResidualEstimator(geom, order=order) as est:
        eta2, total = est.estimate(Z, F, p=1.5)
        r = est.strong_residual(Z, F, p=1.5)
        e1, t1 = m.residual_estimator(geom, Z, F, p=1.5, order=order)
        assert np.array_equal(e1, eta2) and np.array_equal(t1, total)
        assert np.array_equal(m.strong_residual(geom, Z, F, p=1.5, order=order), r)
        ind_owned = est.faces.indicator(Z, p=1.5)
        ind_shot = m.jump_indicator(geom, Z, p=1.5)
        for a, b in ((ind_owned, ind_alone), (ind_shot, ind_alone)):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        with m.Quadrature(geom, order=order) as q:
            w1p_after = q.integrate(Z, kind="w1p", p=1.5, per_element=True)
            assert np.array_equal(w1p_after[0], w1p_before[0]) and np.array_equal(w1p_after[1], w1p_before[1])
            assert np.array_equal(q.integrate(Z, kind="energy", p=1.5, source=F), energy_before)
            assert np.array_equal(q.points(), est.points())                    # the same chains of fused multiply-adds
        t = est.last_times()
        assert t["element_ms"] > 0 and t["reduce_ms"] >= 0


# ---- 5. refusals on the device, and the lifecycle ---------------------------------------------------------------------

def test_an_inverted_element_is_refused():
    geom = m.subdivide(m.fem2d(k=1), 2)
    x = geom.x.copy()
    x[[0, 1], 2, :] = x[[1, 0], 2, :]
    x[[2, 3], 2, :] = x[[3, 2], 2, :]              # element 2 with its first axis reversed: det J < 0, same node ids
    bad = dataclasses.replace(geom, x=x)
    with pytest.raises(ValueError, match="residual: det J is not positive and finite at a point of element 2"):
        m.ResidualEstimator(bad)
    with pytest.raises(ValueError, match="det J is not positive and finite"):
        m.strong_residual(bad, np.zeros(16), np.zeros(16))


def test_lifecycle():
    geom = m.subdivide(m.fem2d(k=2), 2)
    z, f = RT.data(geom, 1)
    z = z[:, 0]
    est = m.ResidualEstimator(geom)
    with pytest.raises(m.device.MGBHipError, match="no pointwise or integrate call"):
        est.last_times()
    v = est.estimate(z, f)
    assert est.points().shape == (4, 16, 2) and est.weights().shape == (4, 16) and est.element_sizes().shape == (4,)
    assert abs(est.weights().sum() - 4.0) <= 64 * EPS and np.all(np.abs(est.element_sizes() - 1.0) <= 64 * EPS)
    with pytest.raises(ValueError, match="ResidualEstimator: .*source at points"):
        est.interior(z, np.zeros((4, 15)))
    with pytest.raises(ValueError, match="ResidualEstimator: .*finite and >= 1"):
        est.strong_residual(z, f, p=0.99)
    est.close()
    est.close()
    assert est.closed and est.faces.closed
    for call in (lambda: est.strong_residual(z, f), lambda: est.interior(z, f), lambda: est.estimate(z, f), est.points,
                 est.weights, est.element_sizes, est.last_times):
        with pytest.raises(ValueError, match="ResidualEstimator: the estimator is closed"):
            call()
    with m.ResidualEstimator(geom) as e2:
        v2 = e2.estimate(z, f)
        assert np.array_equal(v2[0], v[0]) and v2[1] == v[1]
    assert e2.closed
