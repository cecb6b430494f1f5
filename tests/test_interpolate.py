"""interpolate() on the CPU: argument errors raised before any device work, the P1 / P2 basis tables the device
evaluates, and the reference-triangle tables left as they were."""
from fractions import Fraction

import numpy as np
import pytest

import mgb_amd as m
from mgb_amd import fem2d_p1, fem2d_p2


def _nvals(geom):
    return geom.x.shape[0] * geom.x.shape[1]


@pytest.mark.parametrize("geom,name", [
    (m.fem1d(nodes=np.linspace(-1, 1, 4), k=2), "fem1d"),
    (m.fem2d(k=2), "fem2d"),
    (m.fem3d(k=1), "fem3d"),
    (m.fem2d_P1(), "fem2d_P1"),
    (m.fem2d_P2(), "fem2d_P2"),
    (m.spectral1d(n=8), "spectral1d"),
    (m.spectral2d(n=4), "spectral2d"),
])
def test_wrong_length_names_the_expected_count(geom, name):
    n = _nvals(geom)
    d = geom.x.shape[2]
    pts = 0.1 if d == 1 else np.zeros((2, d))
    with pytest.raises(ValueError, match=rf"^{name} interpolation needs {n} values \(got {n + 1}\)$"):
        m.interpolate(geom, np.zeros(n + 1), pts)
    with pytest.raises(ValueError, match=rf"needs {n} values \(got {n - 1}\)"):
        m.interpolate(geom, np.zeros((n - 1, 3)), pts)


@pytest.mark.parametrize("geom", [m.fem2d(k=1), m.fem3d(k=1), m.fem2d_P1(), m.fem2d_P2(), m.spectral2d(n=4)])
def test_point_width_must_be_d(geom):
    d = geom.x.shape[2]
    z = np.zeros(_nvals(geom))
    for bad in (np.zeros((3, d + 1)), np.zeros(d + 1), np.zeros((2, 3, d)), 0.5):
        with pytest.raises(ValueError, match=rf"M-by-{d} array"):
            m.interpolate(geom, z, bad)


def test_embedded_manifold_is_refused():
    geom = m.fem1d(K=np.array([[[0.0, 0.0]], [[1.0, 1.0]]]), ambient=2)     # a segment in the plane
    with pytest.raises(ValueError, match="embedded manifolds"):
        m.interpolate(geom, np.zeros(_nvals(geom)), np.zeros((1, 2)))


@pytest.mark.parametrize("bubble", [True, False])
def test_curved_p2_is_refused(bubble):
    geom = m.fem2d_P2(bubble=bubble)
    K = geom.x.copy()
    slot = 6 if bubble else 3
    K[slot, 0, 0] += 1e-9 * (1 + abs(K[slot, 0, 0]))      # one edge (or the bubble) node off its straight position
    g = m.fem2d_P2(bubble=bubble, K=K)
    with pytest.raises(ValueError, match="straight elements"):
        m.interpolate(g, np.zeros(_nvals(g)), np.zeros((1, 2)))


def test_nonfinite_mesh_is_refused():
    K = m.fem2d_P1().x.copy()
    geom = m.fem2d_P1(K=K)
    geom.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node"):
        m.interpolate(geom, np.zeros(_nvals(geom)), np.zeros((1, 2)))


def _mono(l1, l2):
    return np.array([l1 ** i * l2 ** j for i, j in fem2d_p2.MONOMIALS])


# (l1, l2) of the nodes of each table: P1 corners slot 0, 1, 2; P2 from the barycentric node rows (l1, l2, l3)
@pytest.mark.parametrize("table,nodes", [
    (fem2d_p1.basis_coefficient_table(), [(1.0, 0.0), (0.0, 1.0), (0.0, 0.0)]),
    (fem2d_p2.basis_coefficient_table(True), [tuple(r[:2]) for r in fem2d_p2.reference_triangle(True)["K"]]),
    (fem2d_p2.basis_coefficient_table(False), [tuple(r[:2]) for r in fem2d_p2.reference_triangle(False)["K"]]),
])
def test_basis_tables_are_nodal_and_a_partition_of_unity(table, nodes):
    assert table.shape == (len(nodes), 10)
    A = np.array([[table[j] @ _mono(*nodes[i]) for j in range(len(nodes))] for i in range(len(nodes))])
    assert np.abs(A - np.eye(len(nodes))).max() <= 1e-15
    rng = np.random.default_rng(3)
    for l1, l2 in rng.random((200, 2)):
        assert abs(table @ _mono(l1, l2)).sum() > 0
        assert abs((table @ _mono(l1, l2)).sum() - 1.0) <= 1e-14


def _reference_triangle_parent(bubble):
    """The construction reference_triangle carried inline before it was factored out (rational arithmetic)."""
    nodes = fem2d_p2._bary_nodes(bubble)
    V = len(nodes)
    one = Fraction(1)
    l1, l2 = {(1, 0): one}, {(0, 1): one}
    l3 = {(0, 0): one, (1, 0): -one, (0, 1): -one}
    mul = fem2d_p2._poly_mul
    mons = [{(0, 0): one}, l1, l2, mul(l1, l1), mul(l1, l2), mul(l2, l2)]
    if bubble:
        mons.append(mul(mul(l1, l2), l3))
    ev = fem2d_p2._poly_eval
    Vand = [[ev(mo, nd[0], nd[1]) for mo in mons] for nd in nodes]
    eye = [[one if i == j else 0 * one for j in range(V)] for i in range(V)]
    coef = fem2d_p2._solve_exact(Vand, eye)
    basis = []
    for j in range(V):
        pj = {}
        for mm in range(V):
            for key, c in mons[mm].items():
                pj[key] = pj.get(key, 0) + coef[mm][j] * c
        basis.append(pj)
    diff = fem2d_p2._poly_diff
    dx = np.array([[float(ev(diff(basis[j], 0), nd[0], nd[1])) for j in range(V)] for nd in nodes])
    dy = np.array([[float(ev(diff(basis[j], 1), nd[0], nd[1])) for j in range(V)] for nd in nodes])
    w = np.array([float(2 * fem2d_p2._poly_int(basis[j])) for j in range(V)])
    K = np.array([[float(v) for v in nd] for nd in nodes])
    return dict(K=K, w=w, dx=dx, dy=dy)


@pytest.mark.parametrize("bubble", [True, False])
def test_reference_triangle_is_bitwise_unchanged(bubble):
    old = _reference_triangle_parent(bubble)
    new = fem2d_p2.reference_triangle(bubble)
    assert sorted(new) == sorted(old)
    for key in old:
        assert new[key].dtype == old[key].dtype and np.array_equal(new[key], old[key]), key
    # and the literal values the reference tabulates for the weights (src/fem2d_P2.jl:109-128)
    if bubble:
        assert np.array_equal(new["w"] * 60, [3, 8, 3, 8, 3, 8, 27])
    else:
        assert np.array_equal(new["w"] * 3, [0, 1, 0, 1, 0, 1])


def test_interpolate_is_exported():
    from mgb_amd.interpolate import interpolate
    assert m.interpolate is interpolate


@pytest.mark.parametrize("make,L", [(lambda: m.fem2d_P1(), 4), (lambda: m.fem2d_P2(bubble=False), 4),
                                    (lambda: m.fem2d(k=2), 3), (lambda: m.fem3d(k=2), 3)])
def test_hierarchies_number_the_full_level_alike(make, L):
    """The nested-mesh GPU test lifts level-l `:full` coefficients by geometric_mg(g0, L - 1) and geometric_mg(g0, L):
    both lifts of level l's node coordinates must be the node coordinates of their own fine meshes."""
    g0 = make()
    lvl = L - 2
    xl = m.subdivide(g0, lvl + 1).xflat
    for LL in (L - 1, L):
        R = m.geometric_mg(g0, LL).R["full"][lvl]
        assert R.shape[1] == xl.shape[0]
        assert np.abs(R @ xl - m.subdivide(g0, LL).xflat).max() <= 1e-14
