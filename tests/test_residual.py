"""ResidualEstimator without a device: the second-derivative tables against exact arithmetic, every refusal, the launch
plan, the twin against manufactured solutions, and the gradients the p != 2 device comparisons rely on.

The tolerance of the table test.  `sum_i v_i d2phi_i` is formed in exact arithmetic from the float64 table and compared
with the exact second derivative of the polynomial the v_i are the nodal values of, so the difference is the rounding of
the table entries and of the v_i, both relative: `tol = c u sum_i |v_i| |d2phi_i|`, u = eps / 2, with c counted from the
product form, to first order, every entry taken against its own size:

  Q_k, per axis (s = k + 1 nodes), the worst factor L'':  the denominator, k differences and k - 1 products: 2k - 1;
       a term, a product of k - 2 differences: 2 (k - 2) - 1 (0 below k = 3);  the k (k - 1) terms added: k (k - 1) - 1;
       the division: 1.    c_axis = k^2 + 3k - 6 (k >= 3), k^2 + k - 1 below.
       d axes multiplied: d c_axis + d - 1.      c = d c_axis + d - 1 + 1 (the rounding of v_i)
  triangles: a monomial's second derivative, at most 3 products and the integer factor: 4; the row of the coefficient
       table times it, at most 7 non-zero monomials: 7 products and 6 additions: 13.    c = 4 + 13 + 1

Nothing in c comes from an observed error.
"""
import math
import sys

import mpmath
import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.estimate  # noqa: F401
import mgb_amd.faces  # noqa: F401
import mgb_amd.integrate  # noqa: F401
import residual_twin as RT

E = sys.modules["mgb_amd.estimate"]
I = sys.modules["mgb_amd.integrate"]
Fm = sys.modules["mgb_amd.faces"]
EPS = float(np.finfo(np.float64).eps)
MP = RT.MP
mpf = MP.mpf


# ---- d2phi against exact arithmetic --------------------------------------------------------------------------------

def _pderiv(coef, t, n):
    """The n-th derivative at t of sum_j coef[j] t^j, in mp."""
    c = [mpf(v) for v in coef]
    for _ in range(n):
        c = [j * c[j] for j in range(1, len(c))]
    return MP.fsum(cj * t ** j for j, cj in enumerate(c)) if c else mpf(0)


def _qk_polynomial(d, k):
    """Two products of per-axis polynomials of degree k: a member of Q_k that is no product itself.  Returns the
    function (point as mpf list, derivative orders per axis) -> value."""
    rng = np.random.default_rng(100 * d + k)
    coef = [[[float(v) for v in rng.integers(-4, 5, k + 1) / 4.0] for _ in range(d)] for _ in range(2)]
    for term in coef:
        for row in term:
            row[k] = 1.0 if row[k] == 0.0 else row[k]                 # the full degree on every axis

    def f(pt, orders):
        return MP.fsum(MP.fprod(_pderiv(term[a], pt[a], orders[a]) for a in range(d)) for term in coef)
    return f


def _qk_constant(d, k):
    c_axis = (2 * k - 1) + max(2 * (k - 2) - 1, 0) + (k * (k - 1) - 1) + 1
    return d * c_axis + d - 1 + 1


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("d", [2, 3])
def test_qk_second_derivative_tables_against_exact_arithmetic(d, k):
    geom = m.fem2d(k=k) if d == 2 else m.fem3d(k=k)
    order = 2 if (d == 3 and k == 8) else None          # 729 nodes: a small rule keeps the table build short
    tb = E.residual_tables(geom, order)
    nodes = I.reference_rule(geom, rule="nodal")["xi"]
    f = _qk_polynomial(d, k)
    v = np.array([float(f([mpf(float(t)) for t in nd], [0] * d)) for nd in nodes])
    pairs = E.second_index_pairs(d)
    assert tb["d2phi"].shape == (tb["xi"].shape[0], (k + 1) ** d, len(pairs))
    c, worst = _qk_constant(d, k), 0.0
    for q, pt in enumerate(tb["xi"]):
        ptm = [mpf(float(t)) for t in pt]
        for mth, (b, cc) in enumerate(pairs):
            orders = [(a == b) + (a == cc) for a in range(d)]
            got = MP.fsum(mpf(float(tb["d2phi"][q, i, mth])) * mpf(float(v[i])) for i in range(len(v)))
            tol = c * EPS / 2 * float(np.abs(tb["d2phi"][q, :, mth] * v).sum())
            err = abs(float(got - f(ptm, orders)))
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
            assert err <= tol, (d, k, q, (b, cc), err, tol)
    print(f"Q{k} d={d}: largest error / tolerance {worst:.3e} (c = {c})")


def _triangle_polynomial(p):
    """A polynomial of the family's space over the monomials of fem2d_p2.MONOMIALS: degree 1 (3 nodes), 2 (6 nodes),
    2 plus the cubic bubble l1 l2 (1 - l1 - l2) (7 nodes)."""
    from mgb_amd.fem2d_p2 import MONOMIALS
    coef = dict(zip(MONOMIALS, [0.0] * 10))
    coef.update({(0, 0): 0.5, (1, 0): -1.25, (0, 1): 0.75})
    if p >= 6:
        coef.update({(2, 0): 1.5, (1, 1): -2.0, (0, 2): 0.25})
    if p == 7:
        for mono, c in (((1, 1), 3.0), ((2, 1), -3.0), ((1, 2), -3.0)):
            coef[mono] += c

    def f(pt, orders):
        (i1, i2), out = orders, mpf(0)
        for (a, b), c in coef.items():
            if a >= i1 and b >= i2 and c != 0.0:
                fa = math.factorial(a) // math.factorial(a - i1) * math.factorial(b) // math.factorial(b - i2)
                out += mpf(c) * fa * pt[0] ** (a - i1) * pt[1] ** (b - i2)
        return out
    return f


@pytest.mark.parametrize("name", ["fem2d_P1", "fem2d_P2", "fem2d_P2_nobubble"])
def test_triangle_second_derivative_tables_against_exact_arithmetic(name):
    geom = {"fem2d_P1": m.fem2d_P1, "fem2d_P2": m.fem2d_P2, "fem2d_P2_nobubble": lambda: m.fem2d_P2(bubble=False)}[name]()
    tb = E.residual_tables(geom)
    nodes = I.reference_rule(geom, rule="nodal")["xi"]
    p = nodes.shape[0]
    f = _triangle_polynomial(p)
    v = np.array([float(f([mpf(float(t)) for t in nd], (0, 0))) for nd in nodes])
    assert tb["d2phi"].shape == (tb["xi"].shape[0], p, 3)
    if p == 3:
        assert np.all(tb["d2phi"] == 0.0)                      # exact zeros: the residual of a P1 function is f itself
    c = 4 + 13 + 1
    for q, pt in enumerate(tb["xi"]):
        ptm = [mpf(float(t)) for t in pt]
        for mth, orders in enumerate([(2, 0), (1, 1), (0, 2)]):
            got = MP.fsum(mpf(float(tb["d2phi"][q, i, mth])) * mpf(float(v[i])) for i in range(p))
            tol = c * EPS / 2 * float(np.abs(tb["d2phi"][q, :, mth] * v).sum())
            err = abs(float(got - f(ptm, orders)))
            assert err <= tol, (name, q, orders, err, tol)


def test_tables_reuse_the_rule_of_integrate():
    geom = m.fem2d(k=2)
    tb, ref = E.residual_tables(geom, 3), I.reference_rule(geom, 3, "gauss")
    for key in ("xi", "w", "phi", "dphi"):
        assert np.array_equal(tb[key], ref[key])
    assert tb["order"] == 3 and E.residual_tables(geom)["order"] == 4          # the default is k + 2


# ---- the twin against manufactured solutions -------------------------------------------------------------------------

def _parallelogram(k):
    g = m.subdivide(m.fem2d(k=k), 2)
    A = np.array([[1.0, 0.35], [-0.2, 0.8]])
    return m.fem2d(k=k, K=g.x @ A.T)


def test_twin_residual_of_a_quadratic_on_an_affine_mesh_vanishes():
    """u = x^2 - 0.5 x y + 2 y^2 is in Q_2 on a parallelogram mesh: tr H = 6 at every point, so f = -6 leaves rounding."""
    geom = _parallelogram(2)
    x, tb = RT.tables(geom)
    X = geom.xflat
    z = X[:, 0] ** 2 - 0.5 * X[:, 0] * X[:, 1] + 2.0 * X[:, 1] ** 2
    ex = RT.Exact(x, tb)
    fld = ex.fields(z, np.full((ex.N, ex.Q), -6.0))
    r, A = ex.residual(fld, 2.0)
    c = _qk_constant(2, 2) + 4            # the tables' roundings and those of z = fl(u(x_i)), three operations a term
    for key, v in r.items():
        assert abs(float(v)) <= c * EPS / 2 * A[key], (key, float(v), A[key])


def test_twin_hessian_of_the_coordinates_vanishes_on_a_curved_mesh():
    """u = x_a has the Hessian 0 whatever the map: the correction by H_xi(x_a) removes what H_xi(z) sees."""
    mk, order = RT.cases(m)["fem2d_P2"]
    geom = mk()
    x, tb = RT.tables(geom, order)
    ex = RT.Exact(x, tb)
    fld = ex.fields(geom.xflat, np.zeros(geom.xflat.shape[0]))
    for H in fld["H"].values():
        assert max(abs(float(v)) for v in H) <= 1e-40


@pytest.mark.parametrize("name", sorted(RT.cases(m)))
def test_gradients_of_the_device_cases_stay_away_from_zero(name):
    mk, order = RT.cases(m)[name]
    geom = mk()
    x, tb = RT.tables(geom, order)
    Z, _ = RT.data(geom, ncol=5)
    gn = RT.gradient_norms(x, tb, Z)
    print(f"{name}: min |grad u| = {gn.min():.3f}")
    assert gn.min() > 0.5


# ---- the plan ----------------------------------------------------------------------------------------------------------

PLAN_SHAPES = [(2, 4, 9, 16), (2, 9, 16, 17), (2, 16, 25, 4), (2, 3, 9, 8), (2, 7, 16, 8), (3, 8, 343, 8), (3, 27, 64, 8),
               (3, 27, 125, 8), (3, 64, 216, 100), (3, 729, 8, 5)]


@pytest.mark.parametrize("d,p,Q,N", PLAN_SHAPES)
def test_plan_obeys_the_constants_of_the_lane_plan(d, p, Q, N):
    pl, qp = E.plan(d, p, Q, N), I.plan(d, d, p, Q, N)
    rows = 1 + d + d * (d + 1) // 2
    assert pl["table_bytes"] == rows * Q * p * 8 and qp["table_bytes"] == (1 + d) * Q * p * 8
    for key in ("threads", "S", "G", "chunk", "reduce_threads", "groups"):
        assert pl[key] == qp[key], key                              # the base is Quadrature's
    assert pl["threads"] == 256 and pl["chunk"] == 4 and pl["S"] == min(Q, 256) and 1 <= pl["G"] <= 32
    even = lambda n: (n + 1) & ~1
    G = pl["G"]
    base = 8 * (even(G * p * d) + even(G * p * 4) + even(G * p) + 4 * 256)
    assert G == 1 or base <= 48 * 1024
    assert pl["tables_lds"] == (1 if base + pl["table_bytes"] <= 160 * 1024 else 0)
    assert pl["lds"] == base + (pl["table_bytes"] if pl["tables_lds"] else 0) <= 160 * 1024
    assert qp["lds"] == base + (qp["table_bytes"] if qp["tables_lds"] else 0)
    assert pl["grid"] == min(pl["groups"], 256 if pl["lds"] > 64 * 1024 else 2048)


def test_plan_gate_between_order_4_and_5_of_fem3d_k2():
    assert E.plan(3, 27, 64, 8)["tables_lds"] == 1 and E.plan(3, 27, 64, 8)["table_bytes"] == 138240
    assert E.plan(3, 27, 125, 8)["tables_lds"] == 0 and E.plan(3, 27, 125, 8)["table_bytes"] == 270000
    assert I.plan(3, 3, 27, 125, 8)["tables_lds"] == 1 and I.plan(3, 3, 27, 125, 8)["table_bytes"] == 108000


def test_quadrature_and_faces_plans_are_what_they_were():
    """The values `mgbhip_quadrature_plan` and `mgbhip_faces_plan` reported before quad_lds_tables took its row count."""
    assert I.plan(2, 2, 7, 16, 131072) == dict(threads=256, S=16, G=16, chunk=4, tables_lds=1, reduce_threads=1024,
                                               groups=8192, grid=2048, lds=14464 + 2688, table_bytes=2688)
    assert I.plan(3, 3, 64, 125, 4096)["table_bytes"] == 256000 and I.plan(3, 3, 64, 125, 4096)["tables_lds"] == 0
    fp = Fm.plan(3, 27, 16, 6, 2, 1000)
    assert fp["table_bytes"] == 6 * 4 * 16 * 27 * 8 and fp["tables_lds"] == 1


# ---- refusals, all before any device work ----------------------------------------------------------------------------

def test_unsupported_families_raise_their_own_message():
    for geom, text in [(m.fem1d(nodes=np.linspace(-1, 1, 4)), "fem1d is not supported"),
                       (m.spectral1d(n=6), "spectral1d"),
                       (m.spectral2d(n=4), "spectral2d"),
                       (m.fem2d(k=2, K=np.concatenate([m.fem2d(k=2).x, 0.1 * m.fem2d(k=2).x[..., :1] ** 2], axis=2), ambient=3),
                        "embedded meshes are not supported")]:
        for call in (lambda: m.ResidualEstimator(geom), lambda: m.strong_residual(geom, np.zeros(3), np.zeros(3)),
                     lambda: m.residual_estimator(geom, np.zeros(3), np.zeros(3))):
            with pytest.raises(ValueError, match="ResidualEstimator: .*" + text):
                call()


def test_argument_checks_and_their_messages():
    geom = m.subdivide(m.fem2d(k=2), 2)
    n, N, Q = geom.xflat.shape[0], geom.x.shape[1], 16
    z, f = np.zeros(n), np.zeros(n)
    bad = [
        (dict(z=z[:-1], source=f), "has 36 values"),
        (dict(z=np.zeros((n, 2, 2)), source=f), "vector or a matrix"),
        (dict(z=np.zeros((n, 0)), source=f), "no columns"),
        (dict(z=z, source=None), "source=f is needed"),
        (dict(z=z, source=f[:-1]), "element-space source is a vector of 36"),
        (dict(z=z, source=np.zeros((N, Q + 1))), r"source at points\(\) is \(4, 16\)"),
        (dict(z=z, source=np.zeros((Q, N))), r"source at points\(\) is \(4, 16\)"),
        (dict(z=z, source=np.zeros((N, Q, 1))), "got 3 dimensions"),
        (dict(z=z, source=f, p=0.5), "finite and >= 1"),
        (dict(z=z, source=f, p=math.inf), "finite and >= 1"),
        (dict(z=z, source=f, p=math.nan), "finite and >= 1"),
        (dict(z=z, source=f, p="2"), "must be a number"),
        (dict(z=z, source=f, order=0), "order = 0 must be an integer"),
        (dict(z=z, source=f, order=11), "order = 11 must be an integer"),
    ]
    for kw, text in bad:
        with pytest.raises(ValueError, match="ResidualEstimator: .*" + text):
            m.strong_residual(geom, **kw)
        with pytest.raises(ValueError, match="ResidualEstimator: .*" + text):
            m.residual_estimator(geom, **kw)
    with pytest.raises(ValueError, match="Faces: order = 0"):
        m.residual_estimator(geom, z, f, face_order=0)
    with pytest.raises(ValueError, match="Faces: order = 0"):
        m.ResidualEstimator(geom, face_order=0)
    with pytest.raises(ValueError, match="ResidualEstimator: order = 2.5"):
        m.ResidualEstimator(geom, order=2.5)
    x = geom.x.copy()
    x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="ResidualEstimator: .*non-finite node coordinates"):
        m.ResidualEstimator(m.Geometry(geom.discretization, geom.t, x, geom.w, geom.operators))
    with pytest.raises(ValueError, match="ResidualEstimator: .*has no elements"):
        m.ResidualEstimator(m.Geometry(geom.discretization, geom.t[:, :0], geom.x[:, :0, :], geom.w[:0], geom.operators))


def test_exports():
    for name in ("ResidualEstimator", "residual_estimator", "strong_residual"):
        assert hasattr(m, name)
    from mgb_amd import device
    for name in ("create", "geometry", "pointwise", "integrate", "plan", "times", "destroy"):
        assert "mgbhip_residual_" + name in device.EXPORTS
