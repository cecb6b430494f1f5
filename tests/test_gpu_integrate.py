"""integrate() / norm() / Quadrature on the device against the 50-digit evaluation of the same sums
(tests/integrate_twin.py `Exact`), against the setup layer's own `geom.w @ F(geom.operators)`, at every shape the
launch plan branches on, and for the order guarantees.

The bound.  Every comparison with the exact value is `|device - exact| <= c eps A`, eps = 2^-52.  `A` is the integral
`Exact.integrate` returns next to the value: the measure times a majorant of what a rounding error of the integrand is
proportional to.  With `U = sum_i |phi_i z_i|` an error of `u_q` is a multiple of `u U`, and the power moves by
`p |v|^(p-1) dv`, so `|u - g|^p` is measured against `(|u - g| + 1e-3 V)^(p-1) V`, `V = U + |g|` (the 1e-3 V makes the
mean value theorem hold for every `|dv| <= 1e-3 V`): a difference of nearly equal numbers (an error norm) is measured
against the numbers it was formed from.  For the gradient `T = |J|abs,F |g^-1 xi| + |J g^-1|_2 |sum_i |dphi_i| |z_i||`
(`|J|abs = sum_i |x_i| |dphi_i|^T`) takes the place of `U`.  `c` is counted
from the kernel's operations, to first order, in units of the unit roundoff u = eps / 2.  With n the nodes of an
element, D, E the dimensions, c_det = 0, 3, 8 the operations of the closed-form determinant for D = 1, 2, 3, and two
numbers of the mesh and the tables (`Twin.kappa()`, NumPy): kJ = max |J|_F |J|abs,F |g^-1|_2 and kg = max cond_2(g),

  E_u    = n + 1                     u_q is a chain of n fused multiply-adds (gamma_n), then the subtraction of g
  E_meas = D (2n + E) kJ / 2         det g moves by tr(g^-1 dg), |dg| <= (2n + E) u |J| |J|abs (chains of n for J, of E for g);
           + c_det kg^(D-1) / 2      the closed form's own roundings against products as large as |g|^D; sqrt halves both
           + 3                       sqrt, times w_q, times F
  E_grad = 2n                        chains of n in J and in xi = sum_i dphi_i z_i, each against T
           + (2n + E) D kg           g^-1 moves by g^-1 dg g^-1, and |J|_F^2 |g^-1|_2 <= D cond(g)
           + (c_det + 3) kg^D        cofactors, determinant, reciprocal and product of the closed-form inverse, against
                                     |J| |g^-1| |xi| <= kg^(1/2) |J g^-1| |xi|
           + D + E + 1               the two small products g^-1 xi and J (.), the subtraction of G
  E_pow  = 4                         pow to 2 ulp (p = 1 and p = 2 call none and stay below it)

  value   C = n + E_meas
  lp      C = p E_u + E_pow + E_meas                        |v|^p moves by p |v|^(p-1) dv, dv <= E_u u (U + |g|)
  w1p     C = p E_grad + p (E + 1) / 2 + E_pow + E_meas     the E squares and their sum enter through the power p / 2
  energy  C = max(C_w1p + 1, 2n + 1 + E_meas) + 1           the division by p; the product f_q u_q; the subtraction

and the sums add `L = ceil(log2 S) + ceil(Q / S) - 1` roundings per element (the lane's own points, then the halving tree
over S = min(Q, 256) lanes) and 2 for the compensated reduction over the elements:

  c = 1.05 (C + L + 2) / 2,     5 % for the terms of second order; C u < 1e-3 is asserted, which is also what the
                                1e-3 V in the majorant needs.

Nothing in c comes from an observed error.  The largest observed error / bound per family is printed by the tests and
recorded in DESIGN.md section 8.
"""
import math
import sys

import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.integrate  # noqa: F401
from integrate_twin import Exact, Twin, tables

pytestmark = pytest.mark.gpu

I = sys.modules["mgb_amd.integrate"]
EPS = float(np.finfo(np.float64).eps)
PS = (1.0, 1.5, 2.0, 4.0)


def bound_constant(kind, p, tw):
    n, D, E, Q = tw.p, tw.d, tw.e, tw.Q
    kJ, kg = tw.kappa()
    c_det = (0, 0, 3, 8)[D]
    S = min(Q, 256)
    e_meas = D * (2 * n + E) * kJ / 2 + c_det * kg ** (D - 1) / 2 + 3
    e_grad = 2 * n + (2 * n + E) * D * kg + (c_det + 3) * kg ** D + D + E + 1
    c_w1p = p * e_grad + p * (E + 1) / 2 + 4 + e_meas
    C = {"value": n + e_meas, "lp": p * (n + 1) + 4 + e_meas, "w1p": c_w1p,
         "energy": max(c_w1p + 1, 2 * n + 1 + e_meas) + 1}[kind]
    L = math.ceil(math.log2(S)) + math.ceil(Q / S) - 1 if S > 1 else 0
    assert C * EPS / 2 < 1e-3
    return 1.05 * (C + L + 2) / 2


# ---- the meshes ---------------------------------------------------------------------------------------------------

def _warp(x, amp=0.06):
    """A smooth map of the nodes: elements stay valid and conforming, no element map stays affine."""
    y = x.copy()
    s = x.sum(axis=-1)
    for a in range(x.shape[-1]):
        y[..., a] += amp * np.sin(1.3 * s + 0.7 * a) + 0.5 * amp * x[..., (a + 1) % x.shape[-1]] ** 2
    return y


def _fem1d_curve(k, N, e):
    t = np.linspace(0.0, 2.0, N + 1)
    nodes = m.tensorfem._tf_nodes(k)
    tt = t[:-1][None, :] + 0.5 * (nodes[:, None] + 1.0) * np.diff(t)[None, :]          # (k + 1, N)
    xyz = [np.cos(tt), np.sin(tt) * 1.2, 0.4 * tt ** 2][:e]
    return m.fem1d(k=k, K=np.stack(xyz, axis=2), ambient=e)


def _surface(k=2):
    flat = m.subdivide(m.fem2d(k=k), 2)
    x, y = flat.x[:, :, 0], flat.x[:, :, 1]
    return m.fem2d(k=k, K=np.stack([x + 0.1 * y * y, y - 0.05 * x, 0.3 * x * x - 0.2 * x * y + 0.4 * y], axis=2), ambient=3)


def _fem3d(k, N):
    g = m.subdivide(m.fem3d(k=k), 2)
    return m.fem3d(k=k, K=_warp(g.x[:, :N, :], 0.03))


CASES = {
    "fem1d_k4": lambda: m.fem1d(nodes=np.array([-1.0, -0.35, 0.2, 1.0]), k=4),
    "fem2d_k3": lambda: m.fem2d(k=3, K=_warp(m.subdivide(m.fem2d(k=3), 2).x)),
    "fem3d_k2": lambda: _fem3d(2, 3),
    "fem2d_P1": lambda: m.fem2d_P1(K=_warp(m.subdivide(m.fem2d_P1(), 2).x)),
    "fem2d_P2": lambda: m.fem2d_P2(K=_warp(m.subdivide(m.fem2d_P2(), 2).x), curved=True),
    "fem2d_P2_nobubble": lambda: m.fem2d_P2(bubble=False),
    "curve_R2": lambda: _fem1d_curve(3, 3, 2),
    "curve_R3": lambda: _fem1d_curve(2, 4, 3),
    "surface_R3": lambda: _surface(2),
}
ORDERS = {"fem3d_k2": 3}            # the other cases take the default k + 2

_CACHE = {}


def setup(name, rule="gauss", order=None, geom=None, ncol=2):
    """Everything a case is compared against, built once: the geometry, the twin, the exact evaluator, and seeded data
    (Z two columns, a source, and g, G near u, grad u: an error norm's cancellation)."""
    key = (name, rule, order, ncol)
    if key not in _CACHE:
        geom = CASES[name]() if geom is None else geom
        order = order if rule == "nodal" or order is not None else ORDERS.get(name)
        x, ref = tables(geom, order, rule)
        tw = Twin(x, ref)
        rng = np.random.default_rng(len(name) + 7 * tw.Q)
        X = geom.xflat
        base = np.sin(1.7 * X.sum(axis=1)) + 0.3 * X[:, 0] ** 2
        Z = np.stack([base * (1 + 0.25 * c) + 0.05 * rng.standard_normal(X.shape[0]) + 0.1 * c for c in range(ncol)], axis=1)
        src = np.cos(X[:, 0]) + 0.1 * rng.standard_normal(X.shape[0])
        u, grad = tw.fields(Z)
        g = u + 1e-3 * rng.standard_normal(u.shape)
        G = grad[:, :, 0, :] + 1e-3 * rng.standard_normal(grad[:, :, 0, :].shape)
        _CACHE[key] = dict(geom=geom, order=order, rule=rule, tw=tw, ex=Exact(tw), Z=Z, src=src, g=g, G=G, fld=None)
    return _CACHE[key]


def exact_fields(S):
    if S["fld"] is None:
        S["fld"] = S["ex"].fields(S["Z"], S["src"])
    return S["fld"]


def check_against_exact(S, q, kind, p, minus, label, ratios):
    """Device totals and element values of every column of S["Z"] against the exact ones, each within its bound."""
    tw = S["tw"]
    tot, A, elem = S["ex"].integrate(exact_fields(S), kind, p, minus)
    c = bound_constant(kind, p, tw)
    dev, dev_e = q.integrate(S["Z"], kind=kind, p=p, minus=minus, source=S["src"] if kind == "energy" else None,
                             per_element=True)
    assert dev.shape == (S["Z"].shape[1],) and dev_e.shape == (tw.N, S["Z"].shape[1])
    for col in range(S["Z"].shape[1]):
        err = abs(float(tot[col] - float(dev[col])))
        bound = c * EPS * A[col]
        ratios.append(err / bound)
        print(f"{label} kind={kind} p={p} minus={minus is not None} col={col}: err={err:.3e} bound={bound:.3e} ratio={err / bound:.3e}")
        assert err <= bound, (label, kind, p, col, err, bound)
        # an element's value owes nothing to the reduction over the elements: the same constant covers it
        ee = max(abs(float(elem[col][n] - float(dev_e[n, col]))) for n in range(tw.N))
        assert ee <= bound, (label, kind, p, col, "element", ee, bound)


# ---- device against the 50-digit twin: every family, kind, p, both rules, with and without minus ------------------

@pytest.mark.parametrize("rule", ["gauss", "nodal"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_against_the_exact_sums(name, rule):
    S = setup(name, rule)
    ratios = []
    with m.Quadrature(S["geom"], order=S["order"], rule=rule) as q:
        assert q.n_points == S["tw"].Q and q.n_elements == S["tw"].N
        check_against_exact(S, q, "value", 2.0, None, name, ratios)
        for p in PS:
            check_against_exact(S, q, "lp", p, None, name, ratios)
            check_against_exact(S, q, "lp", p, S["g"], name, ratios)
            check_against_exact(S, q, "w1p", p, None, name, ratios)
            check_against_exact(S, q, "w1p", p, S["G"], name, ratios)
            check_against_exact(S, q, "energy", p, None, name, ratios)
    print(f"RATIO {name} {rule}: largest error / bound = {max(ratios):.3e}")


# ---- the setup layer's own arrays as an independent oracle --------------------------------------------------------

ORACLE = ["fem1d_k4", "fem2d_k3", "fem3d_k2", "fem2d_P2", "fem2d_P1", "curve_R3", "surface_R3"]


@pytest.mark.parametrize("name", ORACLE)
def test_nodal_rule_equals_the_setup_layers_weights_and_operators(name):
    """integrate(rule="nodal") == geom.w @ F(geom.operators) / s, s = 2 for fem2d_P2 and 1 otherwise.  The oracle is
    float64 with operation counts like the kernel's (its operators come out of the same J and g^-1), so the two may
    differ by the sum of two bounds."""
    S = setup(name, "nodal")
    geom, tw = S["geom"], S["tw"]
    s = 2.0 if name.startswith("fem2d_P2") else 1.0
    ops = geom.operators
    axes = ("dx", "dy", "dz")[:tw.e]
    fld = exact_fields(S)
    with m.Quadrature(geom, rule="nodal") as q:
        area = q.weights().sum()
        assert abs(area - geom.w.sum() / s) <= 4 * tw.p * tw.N * EPS * area
        for col in range(S["Z"].shape[1]):
            z = S["Z"][:, col]
            grads = np.stack([ops[a].matvec(z) for a in axes], axis=1)
            gn = np.sqrt((grads * grads).sum(axis=1))
            for p in PS:
                for kind, F in [("value", z), ("lp", np.abs(z) ** p), ("w1p", gn ** p), ("energy", gn ** p / p - S["src"] * z)]:
                    want = math.fsum(geom.w * F) / s
                    got = q.integrate(z, kind=kind, p=p, source=S["src"] if kind == "energy" else None)
                    _, A, _ = S["ex"].integrate(fld, kind, p, None)
                    bound = 2 * bound_constant(kind, p, tw) * EPS * A[col]
                    print(f"{name} oracle kind={kind} p={p} col={col}: diff={abs(got - want):.3e} bound={bound:.3e}")
                    assert abs(got - want) <= bound, (name, kind, p, col, got, want)


# ---- shape edges: every size the plan branches on ------------------------------------------------------------------

def _interval(N, k=2, seed=0):
    rng = np.random.default_rng(seed + N)
    nodes = np.concatenate([[0.0], np.cumsum(0.5 + rng.random(N))])
    return m.fem1d(nodes=nodes / nodes[-1] * 2.0 - 1.0, k=k)


def _edge_check(geom, order, kinds=(("lp", 1.5), ("w1p", 4.0)), ncol=1, label=""):
    S = setup(label, "gauss", order, geom=geom, ncol=ncol)
    ratios = []
    with m.Quadrature(geom, order=order) as q:
        pl = q.plan()
        for kind, p in kinds:
            check_against_exact(S, q, kind, p, S["g"] if kind == "lp" else None, label, ratios)
    return pl, S


def test_element_counts_around_the_workgroup():
    """N = 1, G - 1, G, G + 1 with G read from the plan (fem1d k = 2, n = 4: Q = 4)."""
    G = I.plan(1, 1, 3, 4, 1)["G"]
    assert G > 2
    for N in (1, G - 1, G, G + 1):
        pl, _ = _edge_check(_interval(N), 4, label=f"interval_N{N}")
        assert pl["G"] == G and pl["groups"] == -(-N // G)


def test_element_counts_around_the_reduction_block():
    B = I.plan(1, 1, 2, 2, 1)["reduce_threads"]
    for N in (B - 1, B, B + 1):
        _edge_check(_interval(N, k=1), 2, kinds=(("lp", 2.0),), label=f"interval_k1_N{N}")


def test_points_per_element_64_and_above_256():
    pl, _ = _edge_check(_fem3d(1, 5), 4, label="fem3d_k1_n4")             # Q = 64: exactly one wave per element
    assert pl["S"] == 64 and pl["G"] == 4 and pl["groups"] == 2
    pl, _ = _edge_check(_fem3d(1, 2), 7, label="fem3d_k1_n7")             # Q = 343: lanes stride over the points
    assert pl["S"] == 256 and pl["G"] == 1 and pl["tables_lds"] == 1


def test_tables_in_lds_and_through_l2():
    pl, _ = _edge_check(_fem3d(3, 5), 4, kinds=(("w1p", 1.5),), label="fem3d_k3_n4")
    assert pl["tables_lds"] == 1 and pl["lds"] > 64 * 1024 and pl["groups"] == 2          # the over-64 KB opt-in
    pl, _ = _edge_check(_fem3d(4, 1), 5, kinds=(("w1p", 1.5),), label="fem3d_k4_n5")
    assert pl["tables_lds"] == 0 and pl["table_bytes"] == 500000


def test_column_counts_around_the_chunk():
    geom = CASES["fem2d_P2"]()
    chunk = I.plan(2, 2, 7, 16, 8)["chunk"]
    S = setup("fem2d_P2_cols", "gauss", None, geom=geom, ncol=chunk + 1)
    ratios = []
    with m.Quadrature(geom) as q:
        for ncol in (1, chunk, chunk + 1):
            Sn = dict(S, Z=S["Z"][:, :ncol], g=S["g"][:, :, :ncol], fld=None)
            check_against_exact(Sn, q, "lp", 1.5, Sn["g"], f"ncol{ncol}", ratios)
            check_against_exact(Sn, q, "energy", 4.0, None, f"ncol{ncol}", ratios)


# ---- order guarantees ------------------------------------------------------------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_results_are_reproducible_and_independent_of_company():
    S = setup("fem2d_P2_cols", "gauss", None, geom=CASES["fem2d_P2"](), ncol=I.plan(2, 2, 7, 16, 8)["chunk"] + 1)
    Z, geom = S["Z"], S["geom"]
    with m.Quadrature(geom) as q:
        for kind, p, kw in [("value", 2.0, {}), ("lp", 1.5, dict(minus=S["g"])), ("w1p", 4.0, dict(minus=S["G"])),
                            ("energy", 1.5, dict(source=S["src"]))]:
            t1, e1 = q.integrate(Z, kind=kind, p=p, per_element=True, **kw)
            t2, e2 = q.integrate(Z, kind=kind, p=p, per_element=True, **kw)
            t3 = q.integrate(Z, kind=kind, p=p, **kw)
            assert np.array_equal(_bits(t1), _bits(t2)) and np.array_equal(_bits(e1), _bits(e2))     # run to run
            assert np.array_equal(_bits(t1), _bits(t3))                                              # per_element or not
            for j in range(Z.shape[1]):
                kj = dict(kw)
                if kind == "lp":
                    kj["minus"] = S["g"][:, :, j]
                tj, ej = q.integrate(Z[:, j], kind=kind, p=p, per_element=True, **kj)
                assert isinstance(tj, float) and _bits(tj) == _bits(t1[j]) and np.array_equal(_bits(ej), _bits(e1[:, j]))
            one = m.integrate(geom, Z, kind=kind, p=p, **kw)
            assert np.array_equal(_bits(one), _bits(t1))                                             # the one-shot call
        n1 = q.norm(Z, p=1.5, minus=S["g"])
        assert np.array_equal(_bits(n1), _bits(q.integrate(Z, kind="lp", p=1.5, minus=S["g"]) ** (1 / 1.5)))
        assert np.array_equal(_bits(m.norm(geom, Z, p=1.5, minus=S["g"])), _bits(n1))
    # an element's value does not depend on the mesh around it, nor on its place in the workgroup
    a, b = 3, 7
    sub = m.fem2d_P2(K=geom.x[:, a:b, :], curved=True)
    rows = (np.arange(a, b)[:, None] * 7 + np.arange(7)[None, :]).reshape(-1)
    calls = [("lp", 1.5, "minus", S["g"]), ("w1p", 4.0, "minus", S["G"]), ("energy", 1.5, "source", S["src"])]
    with m.Quadrature(geom) as qf:
        full = [qf.integrate(Z, kind=kind, p=p, per_element=True, **{key: val})[1] for kind, p, key, val in calls]
    with m.Quadrature(sub) as qs:
        for (kind, p, key, val), ef in zip(calls, full):
            part = val[rows] if key == "source" else val[a:b]
            _, es = qs.integrate(Z[rows], kind=kind, p=p, per_element=True, **{key: part})
            assert np.array_equal(_bits(es), _bits(ef[a:b])), kind


def test_total_is_the_compensated_sum_of_the_element_values():
    """|total - fsum(per_element)| <= 2 eps |S| + N eps^2 sum |x_e|, on element values spread over many magnitudes."""
    N = 2 * I.plan(1, 1, 2, 2, 1)["reduce_threads"] + 37
    geom = _interval(N, k=1, seed=3)
    X = geom.xflat[:, 0]
    z = np.exp(12.0 * X) * np.sin(40.0 * X)
    with m.Quadrature(geom, order=3) as q:
        for kind, p in [("value", 2.0), ("lp", 4.0), ("w1p", 1.5)]:
            tot, elem = q.integrate(z, kind=kind, p=p, per_element=True)
            ref = math.fsum(elem)
            bound = 2 * EPS * abs(ref) + N * EPS ** 2 * math.fsum(np.abs(elem))
            print(f"compensated {kind}: |total - fsum| = {abs(tot - ref):.3e}, bound {bound:.3e}, "
                  f"plain sum off by {abs(float(np.sum(elem)) - ref):.3e}")
            assert abs(tot - ref) <= bound


# ---- points, weights, the maximum norm, the lifecycle ---------------------------------------------------------------

@pytest.mark.parametrize("name", ["fem2d_k3", "fem2d_P2", "curve_R3", "surface_R3", "fem3d_k2"])
def test_points_and_weights(name):
    S = setup(name, "gauss")
    tw, geom = S["tw"], S["geom"]
    with m.Quadrature(geom, order=S["order"]) as q:
        pts, w = q.points(), q.weights()
    assert pts.shape == tw.points.shape and w.shape == tw.weights.shape
    # x_q is a chain of n products: n u sum_i |phi_i x_i| on each side
    tol = 2 * tw.p * EPS * np.einsum("qi,ina->nqa", np.abs(tw.phi), np.abs(tw.x))
    assert np.all(np.abs(pts - tw.points) <= tol)
    c = bound_constant("value", 1.0, tw)         # E_meas and more
    assert np.all(np.abs(w - tw.weights) <= 2 * c * EPS * np.abs(tw.weights)) and np.all(w >= 0)
    measure = float(sum(S["ex"].meas.values()))
    assert abs(math.fsum(w.ravel()) - measure) <= c * EPS * measure


def test_flat_meshes_have_their_known_measure():
    for geom, measure in [(m.subdivide(m.fem2d_P2(), 3), 4.0), (m.fem3d(k=2), 8.0), (_interval(9), 2.0),
                          (m.subdivide(m.fem2d_P1(), 2), 4.0)]:
        for rule in ("gauss", "nodal"):
            tw = Twin(*tables(geom, None, rule))
            lebesgue = np.abs(tw.phi).sum(axis=1).max()                     # U = sum_i |phi_i| for z = 1
            tol = bound_constant("value", 1.0, tw) * EPS * measure * lebesgue
            with m.Quadrature(geom, rule=rule) as q:
                ones = np.ones(geom.xflat.shape[0])
                assert abs(math.fsum(q.weights().ravel()) - measure) <= tol
                assert abs(q.integrate(ones) - measure) <= tol
                assert q.integrate(ones, kind="w1p", p=1.5) <= 1e-9


@pytest.mark.parametrize("name", ["fem2d_P2", "fem1d_k4", "surface_R3"])
def test_maximum_norm(name):
    S = setup(name, "gauss")
    tw, Z = S["tw"], S["Z"]
    uf = tw.u_fused(Z)                                  # u_q bit for bit as the device forms it
    with m.Quadrature(S["geom"], order=S["order"]) as q:
        got = q.norm(Z, p=np.inf, minus=S["g"])
        want = np.abs(uf - S["g"]).max(axis=(0, 1))
        assert np.array_equal(_bits(got), _bits(want))             # a max reduction loses nothing
        got0 = q.norm(Z[:, 0], p=math.inf)
        assert isinstance(got0, float) and got0 == np.abs(uf[:, :, 0]).max()
        gw = q.norm(Z, p=np.inf, kind="w1p", minus=S["G"])
        mx, _, _ = S["ex"].integrate(exact_fields(S), "w1p", math.inf, S["G"])
        # |grad u - G| at one point: the w1p count at p = 1, against the largest T + |G|
        scale = float(exact_fields(S)["gabs"].max() + np.sqrt((S["G"] ** 2).sum(axis=2)).max())
        c = bound_constant("w1p", 1.0, tw)
        for col in range(Z.shape[1]):
            assert abs(float(mx[col]) - gw[col]) <= c * EPS * scale


def test_lifecycle():
    geom = m.fem2d_P1()
    z = np.arange(6.0)
    q = m.Quadrature(geom)
    v = q.integrate(z)
    q.close()
    q.close()
    for call in (lambda: q.integrate(z), lambda: q.norm(z), q.points, q.weights):
        with pytest.raises(ValueError, match="Quadrature: the quadrature is closed"):
            call()
    with m.Quadrature(geom) as q2:
        with pytest.raises(m.device.MGBHipError, match="no integrate call has completed"):
            q2.last_times()
        assert _bits(q2.integrate(z)) == _bits(v)
        t = q2.last_times()
        assert t["element_ms"] > 0 and t["reduce_ms"] > 0
    assert q2.closed
    with pytest.raises(ValueError, match="the quadrature is closed"):
        q2.integrate(z)
    with pytest.raises(ValueError, match="z has 5"):            # checked before the device is asked anything
        with m.Quadrature(geom) as q3:
            q3.integrate(np.zeros(5))
