"""Faces on the CPU: the host-built tables, the twin against analytic values, the launch plan at every value where
csrc/faces_layout.hpp branches (the library, no device), and the argument checks that run before any device work."""
import sys

import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.faces  # noqa: F401
import faces_cases as cases
from faces_twin import Exact, topology

Fm = sys.modules["mgb_amd.faces"]

FAMILIES = {
    "fem2d_k1": lambda: m.fem2d(k=1), "fem2d_k3": lambda: m.fem2d(k=3), "fem3d_k1": lambda: m.fem3d(k=1),
    "fem3d_k2": lambda: m.fem3d(k=2), "fem2d_P1": lambda: m.fem2d_P1(), "fem2d_P2": lambda: m.fem2d_P2(),
    "fem2d_P2_nobubble": lambda: m.fem2d_P2(bubble=False),
}


def test_the_package_exports_the_feature():
    assert m.Faces is Fm.Faces and m.boundary_flux is Fm.boundary_flux and m.jump_indicator is Fm.jump_indicator


# ---- host tables ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_tables(name):
    geom = FAMILIES[name]()
    d = geom.x.shape[2]
    tb = Fm.face_tables(geom)
    F, Qf, p = tb["phi"].shape
    assert F == (3 if "P" in name else 2 * d) and Qf == tb["order"] ** (d - 1) and p == geom.x.shape[0]
    assert tb["dphi"].shape == (F, Qf, p, d) and tb["tangents"].shape == (F, d - 1, d) and tb["normals"].shape == (F, d)
    assert tb["corners"].shape == (F, 2 ** (d - 1)) and tb["perm"].shape == (2 if d == 2 else 8, Qf)
    assert np.abs(tb["phi"].sum(axis=2) - 1.0).max() < 1e-13                    # a partition of unity
    assert np.abs(tb["dphi"].sum(axis=2)).max() < 1e-12
    assert abs(tb["wf"].sum() - 2.0 ** (d - 1)) < 1e-14 and np.all(tb["wf"] > 0)
    for f in range(F):
        xi, nr = tb["xi"][f], tb["normals"][f]
        # on the face: the basis of every node off the face vanishes there, and the points lie in the plane through the
        # face's corners that the reference normal is normal to
        off = [i for i in range(p) if i not in tb["nodes"][f]]
        assert np.abs(tb["phi"][f][:, off]).max(initial=0.0) < 1e-13
        for tg in tb["tangents"][f]:
            assert abs(tg @ nr) < 1e-15
        if "P" in name:
            A = Fm.TRIANGLE_CORNERS[f]
            assert np.abs((xi - A) @ nr).max() < 1e-15 and xi.min() >= 0 and xi.sum(axis=1).max() < 1 + 1e-15
            B = Fm.TRIANGLE_CORNERS[(f + 1) % 3]
            assert abs(np.linalg.norm(nr) - np.linalg.norm(tb["tangents"][f, 0])) < 1e-15
            assert np.allclose(tb["tangents"][f, 0], 0.5 * (B - A)) and nr @ (Fm.TRIANGLE_CORNERS[(f + 2) % 3] - A) < 0
        else:
            a, side = f // 2, f % 2
            assert np.all(xi[:, a] == 2.0 * side - 1.0) and np.abs(xi).max() < 1.0 + 1e-15 and nr[a] == 2.0 * side - 1.0
        # the corner nodes are nodes of the face, and the basis of a corner is 1 at it: phi at the face's end points
        assert set(tb["corners"][f]) <= set(tb["nodes"][f])
    # the local faces are those of find_boundary on a single element: every node of the face, in its order of faces
    if "P" not in name:
        from mgb_amd.tensorfem import _multi_index
        k = geom.discretization.k
        want = [[lin for lin in range(p) if _multi_index(lin, k + 1, d)[a] == layer] for a in range(d) for layer in (0, k)]
        assert tb["nodes"] == want


def _corner_params(c, nfa):
    return np.array([2.0 * ((c >> j) & 1) - 1.0 for j in range(nfa)])


@pytest.mark.parametrize("d,n", [(2, 1), (2, 4), (2, 5), (3, 1), (3, 3), (3, 4)])
def test_every_permutation_code_maps_the_points_as_the_corner_relabelling_says(d, n):
    """Code -> where L's corners sit among R's corners -> the multilinear map of the face parameters that this relabelling
    of the corners is -> the R point under every L point."""
    from mgb_amd.integrate import gauss_rule_cube
    s, _ = gauss_rule_cube(d - 1, n)
    perm = Fm.point_permutations(d, n)
    nfa, NC = d - 1, 2 ** (d - 1)
    assert perm.shape == (2 if d == 2 else 8, n ** nfa)
    for code in range(perm.shape[0]):
        assert sorted(perm[code]) == list(range(n ** nfa))
        if d == 2:
            place = [code, 1 - code]                                     # R's corner under L's corner c
        else:
            i0, mm = code // 2, code % 2
            i1 = i0 ^ (1 if mm == 0 else 2)
            i2 = i0 ^ (2 if mm == 0 else 1)
            place = [i0, i1, i2, i0 ^ 3]
        for q in range(n ** nfa):
            w = [np.prod([(1 + _corner_params(c, nfa)[j] * s[q, j]) / 2 for j in range(nfa)]) for c in range(NC)]
            sR = sum(w[c] * _corner_params(place[c], nfa) for c in range(NC))
            assert np.abs(s[perm[code, q]] - sR).max() < 1e-15, (code, q)


@pytest.mark.parametrize("d,k", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_matched_points_coincide_in_every_relative_orientation(d, k):
    """The 4 (2-D) or 24 (3-D) two-element meshes: the setup layer glues (k + 1)^(d-1) nodes, the interior face gets its
    code from the corner ids, and perm[code] pairs each L point with the R point at the same place."""
    codes = set()
    for R in cases.rotations(d):
        geom = cases.pair(d, k, R)
        assert len(np.unique(geom.t)) == 2 * (k + 1) ** d - (k + 1) ** (d - 1)
        tb = Fm.face_tables(geom)
        bnd, itr, ori, ef = topology(geom.t, tb["corners"])
        assert itr.shape == (1, 4) and bnd.shape == (4 * d - 2, 2) and itr[0, 0] == 0 and itr[0, 2] == 1 and itr[0, 1] == 1
        eL, fL, eR, fR = itr[0]
        xL = np.einsum("qi,ia->qa", tb["phi"][fL], geom.x[:, eL, :])
        xR = np.einsum("qi,ia->qa", tb["phi"][fR], geom.x[:, eR, :])
        assert np.abs(xL - xR[tb["perm"][ori[0]]]).max() < 1e-14
        assert np.abs(xL[:, 0] - 1.0).max() < 1e-14
        codes.add(int(ori[0]))
    assert len(cases.rotations(d)) == (4 if d == 2 else 24)
    assert codes == set(range(2 if d == 2 else 8)) or (d == 2 and codes == {1})       # 3-D: every one of the 8 codes occurs


# ---- the twin against analytic values -------------------------------------------------------------------------------

def _exact(geom, order=None):
    tb = Fm.face_tables(geom, order)
    return Exact(geom.x, tb), tb, topology(geom.t, tb["corners"])


def test_twin_boundary_measures():
    for geom, want in [(m.fem2d(k=1), 8.0), (m.fem3d(k=1), 24.0), (m.subdivide(m.fem2d_P2(), 2), 8.0)]:
        ex, tb, (bnd, itr, ori, ef) = _exact(geom)
        assert abs(ex.measures(bnd).sum() - want) < 1e-13


def test_twin_laplace_fluxes():
    for geom, want in [(m.fem2d(k=2), 24.0), (m.fem3d(k=2), 96.0), (m.fem2d_P2(), 24.0)]:
        X = geom.xflat
        u = X[:, 0] ** 2 + 2.0 * X[:, 1] ** 2 + (3.0 * X[:, 2] ** 2 if X.shape[1] == 3 else 0.0)
        ex, tb, (bnd, itr, ori, ef) = _exact(geom)
        tot, A, _, _ = ex.boundary(bnd, u, "flux", 2.0)
        assert abs(float(tot[0]) - want) < 1e-12 and A[0] >= want
        half = np.zeros((len(bnd), tb["wf"].size))
        half[: len(bnd) // 2] = 1.0
        part, _, vals, _ = ex.boundary(bnd, u, "flux", 2.0, weight=half)
        assert abs(float(part[0]) - float(sum(vals[0][: len(bnd) // 2]))) < 1e-30


@pytest.mark.parametrize("d", [2, 3])
def test_twin_kink_jump(d):
    geom = m.subdivide(m.fem2d(k=1) if d == 2 else m.fem3d(k=1), 2)
    ex, tb, (bnd, itr, ori, ef) = _exact(geom)
    z = np.abs(geom.xflat[:, 0])
    on = np.array([np.abs(geom.x[tb["nodes"][fL], eL, 0]).max() < 1e-14 for eL, fL, _, _ in itr])
    assert on.sum() == 2 ** (d - 1)
    for p in (1.0, 1.5, 2.0, 4.0):
        vals, A = ex.jumps(itr, ori, z, "flux", p)
        v = np.array([float(x) for x in vals[0]])
        assert abs(v[on].sum() - 2.0 ** (d + 1)) < 1e-12 and np.abs(v[~on]).max() < 1e-25
        assert min(A[0]) > 0
    vals, _ = ex.jumps(itr, ori, z, "value", 2.0)
    assert max(abs(float(x)) for x in vals[0]) < 1e-30


def test_twin_topology_rejects_three_on_an_edge():
    geom = cases.three_on_an_edge()
    with pytest.raises(ValueError, match="shared by 3 elements"):
        topology(geom.t, Fm.face_tables(geom)["corners"])


# ---- the plan: every value where faces_layout.hpp branches ----------------------------------------------------------

def test_plan_branches():
    P = Fm.plan
    # more points than the largest rule has: refused
    assert P(2, 4, 100, 4, 1, 10)["G"] == 2 and P(2, 4, 101, 4, 1, 10)["G"] == 0
    # faces per workgroup: 256 / Qf, at most 32
    assert P(2, 4, 4, 4, 1, 10)["G"] == 32 and P(2, 4, 8, 4, 1, 10)["G"] == 32 and P(2, 4, 9, 4, 1, 10)["G"] == 28
    assert P(2, 4, 4, 4, 1, 10)["S"] == 4 and P(2, 4, 4, 4, 1, 10)["threads"] == 256 and P(2, 4, 4, 4, 1, 10)["chunk"] == 4
    # ... fewer while nodes + z chunk + partial sums exceed 48 KB: G sides p (d + 4) + 1024 doubles against 6144
    assert P(2, 26, 8, 4, 1, 10)["G"] == 32 and P(2, 26, 8, 4, 1, 10)["lds"] == (32 * 26 * 6 + 1024) * 8 + 4 * 3 * 8 * 26 * 8
    assert P(2, 27, 8, 4, 1, 10)["G"] == 31
    assert P(2, 13, 8, 4, 2, 10)["G"] == 32 and P(2, 14, 8, 4, 2, 10)["G"] == 30            # two sides: twice the nodes
    assert P(3, 64, 25, 6, 2, 100)["G"] == 5 and P(3, 64, 25, 6, 1, 100)["G"] == 10
    # one face alone against the 160 KB cap
    assert P(3, 1389, 4, 6, 2, 10)["G"] == 1 and P(3, 1389, 4, 6, 2, 10)["lds"] == (1389 * 14 + 1024) * 8
    assert P(3, 1390, 4, 6, 2, 10)["G"] == 0
    # the tables: in LDS while everything stays under the cap
    a, b = P(2, 120, 10, 4, 1, 2100), P(2, 121, 10, 4, 1, 2100)
    assert a["G"] == 7 and a["tables_lds"] == 1 and a["table_bytes"] == 115200 and a["lds"] == 48512 + 115200 <= 160 * 1024
    assert b["G"] == 7 and b["tables_lds"] == 0 and b["table_bytes"] == 116160 and b["lds"] == 48848
    assert P(3, 64, 25, 6, 2, 100)["tables_lds"] == 0 and P(3, 64, 25, 6, 2, 100)["table_bytes"] == 307200
    # the grid: the face groups, at most 2048, at most 256 above 64 KB of LDS
    assert a["groups"] == 300 and a["grid"] == 256 and P(2, 120, 10, 4, 1, 7 * 255)["grid"] == 255
    assert b["groups"] == 300 and b["grid"] == 300
    big = P(2, 4, 4, 4, 1, 32 * 3000)
    assert big["groups"] == 3000 and big["grid"] == 2048 and big["lds"] <= 64 * 1024
    assert P(2, 4, 4, 4, 1, 32 * 2048)["grid"] == 2048 and P(2, 4, 4, 4, 1, 32 * 2047 + 1)["grid"] == 2048
    assert P(2, 4, 4, 4, 1, 32 * 2047)["grid"] == 2047
    assert P(2, 4, 4, 4, 2, 0)["groups"] == 0 and P(2, 4, 4, 4, 2, 0)["grid"] == 0 and P(2, 4, 4, 4, 2, 33)["groups"] == 2
    assert P(2, 4, 4, 4, 1, 1)["reduce_threads"] == 1024
    # the shapes DESIGN.md section 8 quotes
    assert P(2, 7, 4, 3, 1, 100)["tables_lds"] == 1 and P(3, 27, 16, 6, 2, 100)["tables_lds"] == 1
    with pytest.raises(m.device.MGBHipError, match="bad sizes"):
        P(1, 4, 4, 4, 1, 10)
    with pytest.raises(m.device.MGBHipError, match="bad sizes"):
        P(2, 4, 4, 4, 3, 10)


# ---- argument errors, all before any device work ----------------------------------------------------------------------

def test_unsupported_families_have_their_own_messages():
    line = m.fem1d(nodes=np.linspace(-1.0, 1.0, 4), k=2)
    tt = np.linspace(0.0, 1.0, 4)
    curve = m.fem1d(k=1, K=np.stack([np.stack([tt[:-1], tt[1:]]), np.stack([tt[:-1] ** 2, tt[1:] ** 2])], axis=2), ambient=2)
    flat = m.fem2d(k=1)
    surf = m.fem2d(k=1, K=np.concatenate([flat.x, 0.1 * flat.x[:, :, :1] ** 2], axis=2), ambient=3)
    seen = []
    for geom, pattern in [(line, "fem1d is not supported"), (curve, "fem1d is not supported"),
                          (surf, "embedded meshes are not supported"), (m.spectral1d(n=4), "spectral1d geometries"),
                          (m.spectral2d(n=4), "spectral2d geometries")]:
        for call in (lambda g=geom: m.Faces(g), lambda g=geom: m.boundary_flux(g, np.zeros(3)),
                     lambda g=geom: m.jump_indicator(g, np.zeros(3))):
            with pytest.raises(ValueError, match=pattern) as e:
                call()
            seen.append(str(e.value))
    assert len(set(seen)) == 4


def test_degree_order_and_call_arguments():
    import mgb_amd.interpolate
    geom = m.fem2d(k=1)
    n = geom.xflat.shape[0]
    z = np.zeros(n)
    for bad in (0, 11, 2.5, True, "3"):
        with pytest.raises(ValueError, match="order = .* must be an integer in 1..10"):
            m.Faces(geom, order=bad)
        with pytest.raises(ValueError, match="order"):
            m.boundary_flux(geom, z, order=bad)
    big = m.fem2d(k=sys.modules["mgb_amd.interpolate"].MAX_DEGREE + 1)
    with pytest.raises(ValueError, match="element degree k = .* is outside"):
        m.Faces(big)
    for call in (m.boundary_flux, m.jump_indicator):
        with pytest.raises(ValueError, match=f"has {n} values \\(z has {n + 1}\\)"):
            call(geom, np.zeros(n + 1))
        with pytest.raises(ValueError, match="vector or a matrix"):
            call(geom, np.zeros((n, 1, 1)))
        with pytest.raises(ValueError, match="no columns"):
            call(geom, np.zeros((n, 0)))
        for p in (0.5, 0.999, np.inf, np.nan, -1.0):
            with pytest.raises(ValueError, match="must be finite and >= 1"):
                call(geom, z, p=p)
        with pytest.raises(ValueError, match="p must be a number"):
            call(geom, z, p="2")
    Qf = 3
    for w in (np.ones(Qf), np.ones((4, Qf + 1)), np.ones((4, Qf, 1))):
        with pytest.raises(ValueError, match=f"weight must be \\(B, {Qf}\\)"):
            m.boundary_flux(geom, z, weight=w)
    sp = Fm._Spec(geom, None)
    with pytest.raises(ValueError, match="weight must be \\(4, 3\\)"):
        sp.check_weight(np.ones((5, 3)), 4)
    with pytest.raises(ValueError, match="kind must be 'value' or 'flux'"):
        sp.check_call(z, "lp", 2.0)
    bad_t = m.fem2d(k=1)
    bad_t.t = -np.asarray(bad_t.t) - 1
    with pytest.raises(ValueError, match="node ids in"):
        m.Faces(bad_t)
    nan_x = m.fem2d(k=1)
    nan_x.x = nan_x.x.copy()
    nan_x.x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="non-finite node coordinates"):
        m.Faces(nan_x)


def test_use_after_close_needs_no_device():
    fc = Fm.Faces.__new__(Fm.Faces)                 # never created: close() frees nothing and closes
    fc.close()
    fc.close()
    assert fc.closed
    for call in (lambda: fc.integrate(np.zeros(4)), lambda: fc.jumps(np.zeros(4)), lambda: fc.indicator(np.zeros(4)),
                 fc.points, fc.normals, fc.measures, fc.interior_measures, fc.face_sizes, fc.boundary_nodes, fc.last_times):
        with pytest.raises(ValueError, match="Faces: the faces are closed"):
            call()
