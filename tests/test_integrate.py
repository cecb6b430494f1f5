"""integrate() / norm() / Quadrature on the host: the rules and basis tables in exact arithmetic, the NumPy twin
(tests/integrate_twin.py) against closed forms, the launch plan, and every argument check with its message.  No GPU."""
from fractions import Fraction
from math import factorial
import sys

import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.integrate  # noqa: F401  (m.integrate is the function; the module is reached through sys.modules)
from integrate_twin import Exact, Twin, tables

I = sys.modules["mgb_amd.integrate"]

# what a float64 rule can owe to the rounding of its own points and weights, relative to the sum of |terms|
RULE_TOL = Fraction(1, 10 ** 13)


def _frac(a):
    return [Fraction(float(v)) for v in np.ravel(a)]


def _cube_moment(m_):          # int_{-1}^{1} x^m dx
    return Fraction(0) if m_ % 2 else Fraction(2, m_ + 1)


def _tri_moment(a, b):         # int over the reference triangle of l1^a l2^b
    return Fraction(factorial(a) * factorial(b), factorial(a + b + 2))


def _rule_moment_1d(t, w, m_):
    terms = [wi * ti ** m_ for ti, wi in zip(t, w)]
    return sum(terms), sum(abs(v) for v in terms)


@pytest.mark.parametrize("n", range(1, I.MAX_ORDER + 1))
def test_gauss_rule_is_positive_and_exact_to_degree_2n_minus_1(n):
    pts, w = I.gauss_rule_cube(1, n)
    assert np.all(w > 0)
    t, wf = _frac(pts), _frac(w)
    for deg in range(2 * n):
        val, mag = _rule_moment_1d(t, wf, deg)
        assert abs(val - _cube_moment(deg)) <= RULE_TOL * max(mag, 1), (n, deg)
    val, mag = _rule_moment_1d(t, wf, 2 * n)
    assert abs(val - _cube_moment(2 * n)) > 1000 * RULE_TOL * mag          # and no further


@pytest.mark.parametrize("d", [2, 3])
def test_tensor_gauss_rule_is_the_product_rule_axis_0_fastest(d):
    n = 3
    t1, w1 = I.gauss_rule_cube(1, n)
    pts, w = I.gauss_rule_cube(d, n)
    assert pts.shape == (n ** d, d) and abs(w.sum() - 2.0 ** d) < 1e-14
    for q in range(n ** d):
        mi = [(q // n ** a) % n for a in range(d)]
        assert np.array_equal(pts[q], [t1[c, 0] for c in mi])
        assert w[q] == np.prod([w1[c] for c in mi])


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 10])
def test_conical_rule_is_positive_and_exact_to_total_degree_2n_minus_1(n):
    pts, w = I.conical_rule_triangle(n)
    assert pts.shape == (n * n, 2) and np.all(w > 0)
    assert np.all(pts >= 0) and np.all(pts.sum(axis=1) <= 1)
    x, y, wf = _frac(pts[:, 0]), _frac(pts[:, 1]), _frac(w)
    assert abs(sum(wf) - Fraction(1, 2)) <= RULE_TOL
    for a in range(2 * n):
        for b in range(2 * n - a):
            val = sum(wi * xi ** a * yi ** b for xi, yi, wi in zip(x, y, wf))
            assert abs(val - _tri_moment(a, b)) <= RULE_TOL, (n, a, b)
    val = sum(wi * xi ** (2 * n) for xi, wi in zip(x, wf))
    assert abs(val - _tri_moment(2 * n, 0)) > 1000 * RULE_TOL * _tri_moment(2 * n, 0)


GEOMS = {
    "fem1d_k4": lambda: m.fem1d(nodes=np.linspace(-1, 1, 4), k=4),
    "fem2d_k3": lambda: m.subdivide(m.fem2d(k=3), 2),
    "fem3d_k2": lambda: m.fem3d(k=2),
    "fem2d_P1": lambda: m.subdivide(m.fem2d_P1(), 2),
    "fem2d_P2": lambda: m.subdivide(m.fem2d_P2(), 2),
    "fem2d_P2_nobubble": lambda: m.fem2d_P2(bubble=False),
}


@pytest.mark.parametrize("name", sorted(GEOMS))
@pytest.mark.parametrize("rule", ["gauss", "nodal"])
def test_basis_tables_partition_unity(name, rule):
    ref = I.reference_rule(GEOMS[name](), rule=rule)
    Q, p = ref["phi"].shape
    assert ref["dphi"].shape == (Q, p, ref["xi"].shape[1]) and ref["w"].shape == (Q,)
    assert np.abs(ref["phi"].sum(axis=1) - 1.0).max() <= 64 * np.finfo(float).eps * np.abs(ref["phi"]).sum(axis=1).max()
    assert np.abs(ref["dphi"].sum(axis=1)).max() <= 64 * np.finfo(float).eps * np.abs(ref["dphi"]).sum(axis=1).max()
    assert np.all(ref["w"] >= 0)
    vol = 0.5 if name.startswith("fem2d_P") else 2.0 ** ref["xi"].shape[1]
    assert abs(ref["w"].sum() - vol) <= 16 * np.finfo(float).eps * vol


def test_gauss_tables_interpolate_the_nodal_basis():
    """phi at the element's own nodes is the identity, and the derivative table there is the geometry's own matrix."""
    from mgb_amd.tensorfem import _tf_reference
    ref = _tf_reference(2, 3)
    phi, dphi = I.qk_tables(2, 3, ref["nodesref"])
    assert np.abs(phi - np.eye(16)).max() < 1e-14
    for b in range(2):
        assert np.abs(dphi[:, :, b] - ref["Daxis"][b]).max() < 1e-12
    from mgb_amd import fem2d_p2
    R = fem2d_p2.reference_triangle(True)
    phi, dphi = I.triangle_tables(fem2d_p2.basis_coefficient_table(True), R["K"][:, :2])
    assert np.abs(phi - np.eye(7)).max() < 1e-14
    assert np.abs(dphi[:, :, 0] - R["dx"]).max() < 1e-13 and np.abs(dphi[:, :, 1] - R["dy"]).max() < 1e-13


@pytest.mark.parametrize("name,degree", [("fem1d_k4", 5), ("fem2d_k3", 3), ("fem3d_k2", 3), ("fem2d_P1", 1), ("fem2d_P2", 3),
                                         ("fem2d_P2_nobubble", 2)])
def test_nodal_rule_is_exact_to_its_documented_degree(name, degree):
    ref = I.reference_rule(GEOMS[name](), rule="nodal")
    xi, w = ref["xi"], _frac(ref["w"])
    d = xi.shape[1]
    cols = [_frac(xi[:, a]) for a in range(d)]
    tri = name.startswith("fem2d_P")

    def defect(expo):
        val = sum(wi * np.prod([cols[a][q] ** expo[a] for a in range(d)]) for q, wi in enumerate(w))
        exact = _tri_moment(*expo) if tri else np.prod([_cube_moment(e_) for e_ in expo])
        return abs(val - exact)

    from itertools import product
    for expo in product(range(degree + 2), repeat=d):
        inside = sum(expo) <= degree if tri else max(expo) <= degree
        if inside:
            assert defect(expo) <= RULE_TOL, (name, expo)
    sharp = (degree + 1,) + (0,) * (d - 1)
    if tri or (degree + 1) % 2 == 0:                # an odd power integrates to zero by symmetry on the cube
        assert defect(sharp) > 1e-6


def test_p2_weights_sum_to_twice_the_area():
    """The factor the nodal rule divides out: fem2d_P2's geom.w sums to 2 |Omega|, every other family's to |Omega|."""
    assert m.fem2d_P2().w.sum() == 8.0 and abs(m.fem2d_P2(bubble=False).w.sum() - 8.0) < 1e-14
    assert abs(m.fem2d_P1().w.sum() - 4.0) < 1e-14 and m.fem2d().w.sum() == 4.0
    ref = I.reference_rule(m.fem2d_P2(), rule="nodal")
    from mgb_amd import fem2d_p2
    assert np.array_equal(ref["w"], 0.5 * fem2d_p2.reference_triangle(True)["w"])


# ---- the twin against closed forms on affine meshes ---------------------------------------------------------------

def _twin(geom, order=None, rule="gauss"):
    x, ref = tables(geom, order, rule)
    return Twin(x, ref)


@pytest.mark.parametrize("name", ["fem2d_k3", "fem2d_P2", "fem2d_P1"])
def test_twin_integrates_monomials_over_the_square(name):
    geom = GEOMS[name]()
    t = _twin(geom)
    X = geom.xflat
    kmax = {"fem2d_k3": 3, "fem2d_P2": 2, "fem2d_P1": 1}[name]
    for a in range(kmax + 1):
        for b in range(kmax + 1):
            if name != "fem2d_k3" and a + b > kmax:
                continue
            tot, elem = t.integrate(X[:, 0] ** a * X[:, 1] ** b, "value")
            exact = float(_cube_moment(a) * _cube_moment(b))
            assert abs(tot[0] - exact) < 1e-13 and abs(elem.sum() - exact) < 1e-13
    assert abs(t.weights.sum() - 4.0) < 1e-13


@pytest.mark.parametrize("p", [2, 4])
def test_twin_lp_norm_of_x_on_the_interval(p):
    geom = GEOMS["fem1d_k4"]()
    t = _twin(geom)
    tot, _ = t.integrate(geom.xflat[:, 0], "lp", float(p))
    assert abs(tot[0] - 2.0 / (p + 1)) < 1e-14
    # an error norm against the exact solution at the points: |x - x| = 0 to rounding
    tot, _ = t.integrate(geom.xflat[:, 0], "lp", float(p), minus=t.points[:, :, 0])
    assert tot[0] < 1e-28


def _parallelogram(k=2):
    o, a, b = np.array([0.1, -0.2, 0.3]), np.array([1.0, 0.5, 0.25]), np.array([-0.25, 1.0, 0.75])
    K = np.stack([o, o + a, o + b, o + a + b])[:, None, :]
    return m.subdivide(m.fem2d(k=k, K=K, ambient=3), 2), a, b


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 4.0])
def test_twin_tangential_gradient_on_a_tilted_parallelogram(p):
    geom, a, b = _parallelogram()
    t = _twin(geom)
    c = np.array([0.7, -1.1, 0.4])
    nrm = np.cross(a, b)
    area = np.linalg.norm(nrm)
    nrm = nrm / area
    Pc = c - (c @ nrm) * nrm
    tot, _ = t.integrate(geom.xflat @ c, "w1p", p)
    assert abs(t.weights.sum() - area) < 1e-13
    assert abs(tot[0] - np.linalg.norm(Pc) ** p * area) < 1e-12
    G = np.broadcast_to(Pc, t.points.shape)
    assert t.integrate(geom.xflat @ c, "w1p", p, minus=G)[0][0] < 1e-12 ** min(p, 2.0)
    src = geom.xflat @ np.array([0.3, 0.2, -0.5])
    tot, _ = t.integrate(geom.xflat @ c, "energy", p, source=src)
    fu = t.integrate((geom.xflat @ c) * src, "value")[0][0]        # a product of two linear functions: inside Q_2
    assert abs(tot[0] - (np.linalg.norm(Pc) ** p * area / p - fu)) < 1e-12


def test_exact_evaluation_agrees_with_the_twin_and_bounds_it():
    geom, _, _ = _parallelogram(k=1)
    t = _twin(geom, order=2)
    ex = Exact(t)
    rng = np.random.default_rng(5)
    Z = rng.standard_normal((geom.xflat.shape[0], 2))
    src = rng.standard_normal(geom.xflat.shape[0])
    g = rng.standard_normal((t.N, t.Q))
    G = rng.standard_normal((t.N, t.Q, 3))
    fld = ex.fields(Z, src)
    for kind, p, minus in [("value", 2.0, None), ("lp", 1.5, g), ("w1p", 4.0, G), ("w1p", 1.0, None), ("energy", 1.5, None)]:
        tot, A, elem = ex.integrate(fld, kind, p, minus)
        ft, fe = t.integrate(Z, kind, p, minus, src if kind == "energy" else None)
        for c in range(2):
            assert abs(float(tot[c]) - ft[c]) <= 1e-13 * A[c] and A[c] >= abs(ft[c])
            assert np.abs(np.array([float(v) for v in elem[c]]) - fe[:, c]).max() <= 1e-13 * A[c]
    mx, _, _ = ex.integrate(fld, "lp", np.inf, g)
    assert abs(float(mx[0]) - t.integrand(Z, "lp", np.inf, g)[:, :, 0].max()) < 1e-14
    # the fused chain is the plain dot product to rounding
    assert np.abs(t.u_fused(Z) - t.fields(Z)[0]).max() < 1e-14


# ---- the launch plan ------------------------------------------------------------------------------------------------

def test_plan_stages_the_tables_while_they_fit():
    small = I.plan(3, 3, 64, 64, 5)            # fem3d k = 3, n = 4: 131 KB of tables
    big = I.plan(3, 3, 125, 125, 1)            # fem3d k = 4, n = 5: 500 KB
    assert small["table_bytes"] == 4 * 64 * 64 * 8 and small["tables_lds"] == 1 and 64 * 1024 < small["lds"] <= 160 * 1024
    assert big["table_bytes"] == 500000 and big["tables_lds"] == 0 and big["lds"] <= 64 * 1024
    for (d, e, p, Q) in [(1, 1, 2, 1), (1, 3, 9, 10), (2, 2, 7, 16), (2, 2, 81, 100), (2, 3, 9, 4), (3, 3, 27, 343),
                         (3, 3, 729, 1000)]:
        pl = I.plan(d, e, p, Q, 1000)
        assert pl["S"] == min(Q, pl["threads"]) and pl["G"] >= 1 and pl["G"] * pl["S"] <= pl["threads"]
        assert pl["lds"] <= 160 * 1024 and pl["groups"] == -(-1000 // pl["G"]) and 1 <= pl["grid"] <= pl["groups"]
        assert pl == {**I.plan(d, e, p, Q, 7), "groups": pl["groups"], "grid": pl["grid"]}       # N moves the grid only


# ---- argument checks: all of them before any device work ----------------------------------------------------------

def test_argument_checks_and_their_messages():
    g = m.fem2d_P2()
    z = np.zeros(14)
    bad = [
        (dict(kind="l2"), "kind must be one of 'value', 'lp', 'w1p', 'energy'"),
        (dict(z=np.zeros(13)), r"a fem2d_P2 function on this mesh has 14 values \(z has 13\)"),
        (dict(z=np.zeros((14, 2, 2))), "z must be a vector or a matrix"),
        (dict(z=np.zeros((14, 0))), "z has no columns"),
        (dict(kind="value", minus=np.zeros((2, 16))), "minus goes with kind='lp' or kind='w1p'"),
        (dict(kind="energy", p=2.0, source=z, minus=np.zeros((2, 16))), "minus goes with kind='lp' or kind='w1p'"),
        (dict(kind="lp", minus=np.zeros((2, 15))), r"minus must hold g at points\(\) as \(2, 16\)"),
        (dict(kind="lp", z=np.zeros((14, 3)), minus=np.zeros((2, 16, 2))), r"as \(2, 16\) or \(2, 16, 3\)"),
        (dict(kind="w1p", minus=np.zeros((2, 16))), r"minus must hold G at points\(\) as \(2, 16, 2\)"),
        (dict(kind="energy"), "kind='energy' needs source=f"),
        (dict(kind="energy", source=np.zeros(13)), "source must be a vector of 14 values"),
        (dict(kind="lp", source=z), "source goes with kind='energy'"),
        (dict(kind="lp", p=0.0), "p = 0.0 must be finite and > 0"),
        (dict(kind="lp", p=-1), "must be finite and > 0"),
        (dict(kind="lp", p=np.inf), "p = inf must be finite and > 0"),
        (dict(kind="lp", p=np.nan), "must be finite and > 0"),
        (dict(kind="lp", p="2"), "p must be a number"),
        (dict(order=0), "order = 0 must be an integer in 1..10"),
        (dict(order=11), "order = 11 must be an integer in 1..10"),
        (dict(order=2.5), "must be an integer in 1..10"),
        (dict(rule="simpson"), "rule must be 'gauss' or 'nodal'"),
        (dict(rule="nodal", order=3), "the nodal rule has the element's own nodes; it takes no order"),
    ]
    for kw, msg in bad:
        kw = dict(kw)
        zz = kw.pop("z", z)
        with pytest.raises(ValueError, match=msg):
            m.integrate(g, zz, **kw)
    with pytest.raises(ValueError, match="norm takes kind='lp' or kind='w1p'"):
        m.norm(g, z, kind="value")
    with pytest.raises(ValueError, match="must be finite and > 0 \\(or inf\\)"):
        m.norm(g, z, p=0)
    with pytest.raises(ValueError, match="z has 13"):
        m.norm(g, np.zeros(13), p=np.inf)


def test_geometry_checks_and_their_messages():
    for geom, name in [(m.spectral1d(4), "spectral1d"), (m.spectral2d(3), "spectral2d")]:
        with pytest.raises(ValueError, match=f"no element quadrature for {name} geometries"):
            m.Quadrature(geom)
        with pytest.raises(ValueError, match=f"no element quadrature for {name}"):
            m.integrate(geom, np.zeros(len(geom.w)))
        with pytest.raises(ValueError, match=f"no element quadrature for {name}"):
            m.norm(geom, np.zeros(len(geom.w)))
    g = m.fem2d_P1()
    empty = m.Geometry(g.discretization, g.t[:, :0], g.x[:, :0, :], g.w[:0], g.operators)
    with pytest.raises(ValueError, match="the fem2d_P1 geometry has no elements"):
        m.Quadrature(empty)
    x = g.x.copy()
    x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node coordinates"):
        m.Quadrature(m.Geometry(g.discretization, g.t, x, g.w, g.operators))
    with pytest.raises(ValueError, match="element degree k = 9 is outside 1..8"):
        m.Quadrature(m.fem1d(k=9))


def test_use_after_close_raises_without_a_device():
    q = m.Quadrature.__new__(m.Quadrature)           # never created: close() has nothing to free
    q.close()
    q.close()
    for call in (lambda: q.integrate(np.zeros(3)), lambda: q.norm(np.zeros(3)), q.points, q.weights):
        with pytest.raises(ValueError, match="Quadrature: the quadrature is closed"):
            call()
