"""Faces on the device: the topology against the dict twin, every relative orientation of two elements, analytic values,
and every face quantity against the 50-digit evaluation of the same sums (tests/faces_twin.py `Exact`), plus the order
guarantees and the lifecycle.

The bound.  Every comparison with the exact value is `|device - exact| <= c eps A`, eps = 2^-52.  `A` is what `Exact`
returns next to the value: the face measure times a majorant of what a rounding error of the integrand is proportional
to.  With `U = sum_i |phi_i z_i|` an error of `u` is a multiple of `u U`; with `T = |J^-1|_2 (|J|abs,F |grad u| +
|sum_i |dphi_i| |z_i - z_0||)` (`|J|abs = sum_i |x_i| |dphi_i|^T`) an error of `grad u` is a multiple of `u T`, and the flux
`a . n = |grad u|^(p-2) grad u . n` is measured against `m = max(1, p-1) (|grad u| +- 1e-3 T)^(p-2) T >= |a|` (`+` for
p >= 2, `-` below: `Exact.majorant`).  A jump is measured against `(U_L + U_R)^2` resp. `(m_L + m_R)^2`: a difference of
nearly equal numbers against the numbers it was formed from.  `c` is counted from the kernel's operations (faces.hip is
compiled with the compiler's default contraction, which only fuses a product into a sum and so removes roundings), to
first order, in units of the unit roundoff u = eps / 2.  With n the nodes of an element, d the dimension,
c_cof = 0, 2 the roundings of a cofactor and c_det = 2, 5 those of the determinant behind it for d = 2, 3, and two numbers
of the mesh and the tables (`Exact.kJ`, `Exact.kappa`): kJ = max |J^-1|_2 |J|abs,F and k = max cond_2(J),

  E_ds   = (d-1) (n kJ + d k)          the images J t_j of the d-1 tangents: J's chains of n against |J|abs |t|, then d
           + c_cof k^2                 products against |J| |t| <= k |J t|; the cross product (3-D)
           + (d+1)/2 + 2               the squares and their sum under the square root, the root, times wf_q
  E_grad = 2n + 2                      the chains of J and of xi = sum_i dphi_i (z_i - z_0) with its subtractions, against T
           + (c_cof + c_det + d + 2) d k^(d-1)
                                       cofactors (|J|^3 / det <= k^2), determinant (|J| |C| / det = k), its reciprocal
                                       and the products C xi / det (|C| |xi| / det <= k |grad u|), d terms in every sum
  E_n    = n kJ + c_cof d k^(d-1)      the direction of C n_ref: J's rounding, the cofactors,
           + d + (d+1)/2 + 2           the product, the squares under the root, the root and the division by it
  E_pow  = 0 (p = 2),  2 + (d+1)/2 (p = 1: root and division),  4 + |p-2| (d+1)/2 (pow to 2 ulp, |grad u|^2 through it)
  C_side = E_grad + E_n + d + E_pow + 1        ... the dot product grad u . n, the product with the power

  boundary value   C = n + E_ds + 2                      u's chain, the weight, the product with ds
  boundary flux    C = C_side + E_ds + 2
  jump value       C = 2 (n + 1) + 1 + E_ds + 1          (j + dj)^2 - j^2 = 2 j dj, |j| <= U_L + U_R, dj <= (n + 1) u (U_L + U_R)
  jump flux        C = 2 (C_side + 1) + 1 + E_ds + 1

and the sums add `L = ceil(log2 Qf)` roundings per face (the halving tree over its Qf lanes) and 2 for the compensated
reduction over the faces:

  c = 1.05 (C + L + 2) / 2,     5 % for the terms of second order; C u < 1e-3 is asserted, which is also what the
                                1e-3 T in the majorant needs.

Nothing in c comes from an observed error.  The largest observed error / bound per family is printed by the tests and
recorded in DESIGN.md section 8.
"""
import math
import sys

import numpy as np
import pytest

import mgb_amd as m
import mgb_amd.faces  # noqa: F401
import faces_cases as cases
from faces_twin import Exact, topology

pytestmark = pytest.mark.gpu

Fm = sys.modules["mgb_amd.faces"]
EPS = float(np.finfo(np.float64).eps)
PS = (1.0, 1.5, 2.0, 4.0)


def bound_constant(what, p, ex):
    """`what` in "bvalue", "bflux", "jvalue", "jflux"; `ex` an `Exact` that has seen every point of the comparison."""
    n, d, Qf = ex.p, ex.d, ex.Qf
    kJ, k = ex.kJ, ex.kappa
    c_cof, c_det = (0, 2) if d == 2 else (2, 5)
    e_ds = (d - 1) * (n * kJ + d * k) + c_cof * k ** 2 + (d + 1) / 2 + 2
    e_grad = 2 * n + 2 + (c_cof + c_det + d + 2) * d * k ** (d - 1)
    e_n = n * kJ + c_cof * d * k ** (d - 1) + d + (d + 1) / 2 + 2
    e_pow = 0 if p == 2 else 2 + (d + 1) / 2 if p == 1 else 4 + abs(p - 2) * (d + 1) / 2
    c_side = e_grad + e_n + d + e_pow + 1
    C = {"bvalue": n + e_ds + 2, "bflux": c_side + e_ds + 2, "jvalue": 2 * (n + 1) + 1 + e_ds + 1,
         "jflux": 2 * (c_side + 1) + 1 + e_ds + 1}[what]
    L = math.ceil(math.log2(Qf)) if Qf > 1 else 0
    assert C * EPS / 2 < 1e-3
    return 1.05 * (C + L + 2) / 2


_CACHE = {}


def setup(name, geom_fn, order=None):
    """The geometry, its tables, the twin's topology and an `Exact`, built once per name."""
    if name not in _CACHE:
        geom = geom_fn()
        tb = Fm.face_tables(geom, order)
        bnd, itr, ori, ef = topology(geom.t, tb["corners"])
        _CACHE[name] = dict(geom=geom, order=order, tb=tb, bnd=bnd, itr=itr, ori=ori, ef=ef, ex=Exact(geom.x, tb), fields={})
    return _CACHE[name]


def _within(label, dev, exact, A, c, ratios):
    err, bound = abs(float(exact - float(dev))), c * EPS * A
    ratios.append(err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
    assert err <= bound, (label, err, bound, float(dev), float(exact))


def check_boundary(S, fc, Z, kind, p, weight, label, ratios, cache):
    ex = S["ex"]
    tot, A, vals, Af = ex.boundary(S["bnd"], Z, kind, p, weight, cache=cache)
    c = bound_constant("b" + kind, p, ex)
    dev, dev_f = fc.integrate(Z, kind=kind, p=p, weight=weight, per_face=True)
    Zc = np.asarray(Z).reshape(len(Z), -1)
    dev, dev_f = np.atleast_1d(dev), np.asarray(dev_f).reshape(len(S["bnd"]), -1)
    for col in range(Zc.shape[1]):
        _within((label, kind, p, col, "total"), dev[col], tot[col], A[col], c, ratios)
        for b in range(len(S["bnd"])):
            _within((label, kind, p, col, "face", b), dev_f[b, col], vals[col][b], Af[col][b], c, ratios)
    print(f"{label} boundary {kind} p={p} weight={weight is not None}: largest error / bound so far {max(ratios):.3e}")


def check_jumps(S, fc, Z, kind, p, label, ratios, cache):
    ex = S["ex"]
    vals, Af = ex.jumps(S["itr"], S["ori"], Z, kind, p, cache=cache)
    c = bound_constant("j" + kind, p, ex)
    dev = np.asarray(fc.jumps(Z, kind=kind, p=p)).reshape(len(S["itr"]), -1)
    for col in range(dev.shape[1]):
        for i in range(len(S["itr"])):
            _within((label, kind, p, col, "face", i), dev[i, col], vals[col][i], Af[col][i], c, ratios)
    print(f"{label} jumps {kind} p={p}: largest error / bound so far {max(ratios):.3e}")
    return dev, vals, Af, c


# ---- topology -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.TOPOLOGY))
def test_topology_equals_the_twin(name):
    S = setup("topo_" + name, cases.TOPOLOGY[name])
    geom = S["geom"]
    with m.Faces(geom) as fc:
        assert fc.n_boundary == len(S["bnd"]) and fc.n_interior == len(S["itr"])
        for key, got in [("bnd", fc.boundary), ("itr", fc.interior), ("ori", fc.orientation), ("ef", fc.element_faces)]:
            assert got.dtype == np.int32 and got.shape == S[key].shape and np.array_equal(got, S[key]), key
        assert 2 * fc.n_interior + fc.n_boundary == fc.n_elements * fc.n_local_faces
        # find_boundary marks every (node, element) whose global id is an end point (P1), a node of a half edge (P2) or
        # a node of a face (Q_k) used once: the ids on the boundary faces, which is this dedup rule for every family
        # (the bubble of a P2 element is never on a face)
        want = m.find_boundary(geom)
        got = fc.boundary_nodes()
        assert got == want and set(got) == set(want) and len(got) > 0


def test_a_face_shared_by_three_elements_is_refused():
    with pytest.raises(ValueError, match="a face is shared by 3 elements"):
        m.Faces(cases.three_on_an_edge())


def test_a_reflected_element_is_refused():
    geom = m.subdivide(m.fem2d(k=1), 2)
    x = geom.x.copy()
    x[[0, 1], 2, :] = x[[1, 0], 2, :]
    x[[2, 3], 2, :] = x[[3, 2], 2, :]              # element 2 with its first axis reversed: det J < 0, same node ids
    import dataclasses
    with pytest.raises(ValueError, match="det J is not positive and finite on a face of element 2"):
        m.Faces(dataclasses.replace(geom, x=x))


# ---- every relative orientation ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,k", [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_every_relative_orientation(d, k):
    ratios, codes = [], set()
    for r, R in enumerate(cases.rotations(d)):
        S = setup(f"pair_{d}_{k}_{r}", lambda: cases.pair(d, k, R), k + 1)
        geom = S["geom"]
        conforming = cases.polynomial(geom.xflat, k)
        broken = cases.broken_field(geom, ncol=1, seed=r)[:, 0]
        with m.Faces(geom, order=k + 1) as fc:
            assert np.array_equal(fc.interior, S["itr"]) and np.array_equal(fc.orientation, S["ori"])
            codes.add(int(fc.orientation[0]))
            cache = {}
            # conforming: the twin's own jumps are those of the rounding of the sampled nodal values, squared: nothing
            # against the bound, so the device's jumps are within the bound of 0
            for kind, p in [("value", 2.0), ("flux", 2.0), ("flux", 4.0)]:
                dev, vals, A, c = check_jumps(S, fc, conforming, kind, p, f"pair{d}k{k}r{r} conforming", ratios, cache)
                assert float(abs(vals[0][0])) <= 1e-6 * c * EPS * A[0][0]
                assert abs(dev[0, 0]) <= (1 + 1e-6) * c * EPS * A[0][0]
            cache = {}
            check_jumps(S, fc, broken, "value", 2.0, f"pair{d}k{k}r{r} broken", ratios, cache)
            check_jumps(S, fc, broken, "flux", 1.5, f"pair{d}k{k}r{r} broken", ratios, cache)
    if d == 3:
        assert codes == set(range(8))                   # every code of the permutation table occurs
    print(f"RATIO orientations d={d} k={k}: largest error / bound = {max(ratios):.3e}")


# ---- exact values -------------------------------------------------------------------------------------------------------

def test_boundary_measures_of_the_square_and_the_cube():
    for name, fn, want in [("square", lambda: m.fem2d(k=1), 8.0), ("cube", lambda: m.fem3d(k=1), 24.0),
                           ("square_P2", lambda: m.subdivide(m.fem2d_P2(), 2), 8.0)]:
        S = setup("measure_" + name, fn)
        ex = S["ex"]
        with m.Faces(S["geom"]) as fc:
            ms, nr, pts = fc.measures(), fc.normals(), fc.points()
            ones = np.ones(S["geom"].xflat.shape[0])
            total = fc.integrate(ones, kind="value")
        want_ms = ex.measures(S["bnd"])
        c = bound_constant("bvalue", 2.0, ex)
        assert np.all(np.abs(ms - want_ms) <= c * EPS * want_ms)
        lebesgue = np.abs(S["tb"]["phi"]).sum(axis=2).max()
        assert abs(math.fsum(ms.ravel()) - want) <= c * EPS * want and abs(total - want) <= c * EPS * want * lebesgue
        # unit outward normals of an axis-parallel box: +-e_a, pointing away from the centre
        assert np.abs(np.abs(nr).sum(axis=2) - 1.0).max() < 1e-14 and np.all(np.einsum("bqa,bqa->bq", nr, pts) > 0.99)


def test_laplace_fluxes_are_24_96_and_24():
    ratios = []
    for name, fn, want in [("q2_square", lambda: m.fem2d(k=2), 24.0), ("q2_cube", lambda: m.fem3d(k=2), 96.0),
                           ("p2_square", lambda: m.fem2d_P2(), 24.0)]:
        S = setup("laplace_" + name, fn)
        X = S["geom"].xflat
        u = X[:, 0] ** 2 + 2.0 * X[:, 1] ** 2 + (3.0 * X[:, 2] ** 2 if X.shape[1] == 3 else 0.0)
        tot, A, _, _ = S["ex"].boundary(S["bnd"], u, "flux", 2.0)
        with m.Faces(S["geom"]) as fc:
            check_boundary(S, fc, u, "flux", 2.0, None, name, ratios, {})
            dev = fc.integrate(u, kind="flux", p=2.0)
            assert abs(dev - m.boundary_flux(S["geom"], u)) == 0.0
        c = bound_constant("bflux", 2.0, S["ex"])
        assert abs(dev - want) <= c * EPS * A[0] + abs(float(tot[0]) - want) and abs(float(tot[0]) - want) < 1e-12


@pytest.mark.parametrize("d", [2, 3])
def test_kink_jump_is_four_times_the_interface(d):
    S = setup(f"kink_{d}", lambda: m.subdivide(m.fem2d(k=1) if d == 2 else m.fem3d(k=1), 2))
    geom, tb, itr = S["geom"], S["tb"], S["itr"]
    z = np.abs(geom.xflat[:, 0])
    on = np.array([np.abs(geom.x[tb["nodes"][fL], eL, 0]).max() < 1e-14 for eL, fL, _, _ in itr])
    want = 4.0 * 2.0 ** (d - 1)
    ratios, cache = [], {}
    with m.Faces(geom) as fc:
        for p in PS:
            dev, vals, A, c = check_jumps(S, fc, z, "flux", p, f"kink{d}", ratios, cache)
            bound_on = sum(c * EPS * A[0][i] for i in np.nonzero(on)[0])
            bound_all = sum(c * EPS * A[0][i] for i in range(len(itr)))
            assert abs(dev[on, 0].sum() - want) <= bound_on + 1e-12
            for i in np.nonzero(~on)[0]:
                assert abs(dev[i, 0]) <= c * EPS * A[0][i]
            # h_F = 1 on this mesh and every interior face belongs to two elements: the sum of eta2 is sum_F h_F J_F
            eta2, total = fc.indicator(z, p=p)
            assert np.abs(fc.face_sizes() - 1.0).max() <= 8 * EPS
            assert abs(total - want) <= 2 * bound_all + 16 * EPS * want + 1e-12


# ---- warped meshes: every kind against the 50-digit values -----------------------------------------------------------

@pytest.mark.parametrize("name", sorted(cases.WARPED))
def test_warped_meshes_against_the_exact_values(name):
    fn, order = cases.WARPED[name]
    S = setup("warped_" + name, fn, order)
    geom = S["geom"]
    Z = cases.broken_field(geom, ncol=2)
    rng = np.random.default_rng(5)
    ratios, cache = [], {}
    with m.Faces(geom, order=order) as fc:
        assert np.array_equal(fc.interior, S["itr"]) and np.array_equal(fc.boundary, S["bnd"])
        W = rng.standard_normal((fc.n_boundary, fc.n_points))
        check_boundary(S, fc, Z, "value", 2.0, None, name, ratios, cache)
        check_boundary(S, fc, Z, "value", 2.0, W, name, ratios, cache)
        check_jumps(S, fc, Z, "value", 2.0, name, ratios, cache)
        for p in PS:
            check_boundary(S, fc, Z, "flux", p, None, name, ratios, cache)
            check_boundary(S, fc, Z, "flux", p, W, name, ratios, cache)
            check_jumps(S, fc, Z, "flux", p, name, ratios, cache)
        ex = S["ex"]
        c = bound_constant("bvalue", 2.0, ex)
        ms, ims = fc.measures(), fc.interior_measures()
        wb, wi = ex.measures(S["bnd"]), ex.measures(S["itr"])
        assert np.all(np.abs(ms - wb) <= c * EPS * wb) and np.all(np.abs(ims - wi) <= c * EPS * wi)
        hF = fc.face_sizes()
        size = np.array([math.fsum(r) for r in wi]) ** (1.0 / (geom.x.shape[2] - 1))
        assert np.all(np.abs(hF - size) <= (c + fc.n_points) * EPS * size)
        pl = fc.plan(1), fc.plan(2)
        assert name != "fem3d_k1" or (pl[0]["G"] == 16 and pl[0]["groups"] == 2)          # 24 boundary faces: 16 + 8
        print(f"{name}: plans {pl}, kJ = {ex.kJ:.2f}, kappa = {ex.kappa:.2f}")
    print(f"RATIO {name}: largest error / bound = {max(ratios):.3e}")


def test_table_paths_and_many_workgroups():
    """Q3 hexahedra: the tables staged above 64 KB of LDS (order 3) and read through L2 (order 4); P1 at L = 4: six
    workgroups of interior faces, the last one partly filled, and exactly one full workgroup of boundary faces."""
    ratios = []
    for order, staged in [(3, 1), (4, 0)]:
        S = setup(f"q3_pair_{order}", lambda: m.fem3d(k=3, K=cases.warp(cases.pair(3, 3, np.eye(3)).x, 0.03)), order)
        z = cases.broken_field(S["geom"], ncol=1)[:, 0]
        with m.Faces(S["geom"], order=order) as fc:
            for sides in (1, 2):
                pl = fc.plan(sides)
                assert pl["tables_lds"] == staged and (pl["lds"] > 64 * 1024) == bool(staged), pl
            cache = {}
            check_boundary(S, fc, z, "flux", 1.5, None, f"q3 order {order}", ratios, cache)
            check_jumps(S, fc, z, "flux", 1.5, f"q3 order {order}", ratios, cache)
    S = setup("p1_L4", lambda: m.fem2d_P1(K=cases.warp(m.subdivide(m.fem2d_P1(), 4).x)), 2)
    z = cases.broken_field(S["geom"], ncol=1)[:, 0]
    with m.Faces(S["geom"], order=2) as fc:
        G = fc.plan(2)["G"]
        assert fc.n_interior == 176 and fc.n_boundary == 32 == G and fc.plan(2)["groups"] == 6 and fc.plan(1)["groups"] == 1
        assert np.array_equal(fc.interior, S["itr"]) and np.array_equal(fc.element_faces, S["ef"])
        cache = {}
        check_boundary(S, fc, z, "flux", 4.0, None, "p1 L4", ratios, cache)
        check_jumps(S, fc, z, "flux", 4.0, "p1 L4", ratios, cache)
    print(f"RATIO table paths and workgroups: largest error / bound = {max(ratios):.3e}")


# ---- zero gradient, the indicator, the order guarantees, the lifecycle ----------------------------------------------

def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_zero_gradient_has_zero_flux_at_p_1():
    for fn in (lambda: cases.WARPED["fem2d_P2"][0](), lambda: cases.WARPED["fem3d_k1"][0]()):
        geom = fn()
        z = np.full(geom.xflat.shape[0], 0.7)
        with m.Faces(geom) as fc:
            for p in (1.0, 1.5, 2.0, 4.0):
                tot, face = fc.integrate(z, kind="flux", p=p, per_face=True)
                assert tot == 0.0 and not np.any(face != 0.0) and not np.any(np.isnan(face))
                assert not np.any(fc.jumps(z, kind="flux", p=p) != 0.0)
                eta2, total = fc.indicator(z, p=p)
                assert total == 0.0 and not np.any(eta2 != 0.0)


@pytest.mark.parametrize("name", ["fem2d_P2", "fem3d_k1"])
def test_indicator_is_the_gather_of_the_jumps(name):
    fn, order = cases.WARPED[name]
    geom = fn()
    Z = cases.broken_field(geom, ncol=3)
    with m.Faces(geom, order=order) as fc:
        J = fc.jumps(Z, kind="flux", p=1.5)
        hF, ef = fc.face_sizes(), fc.element_faces
        eta2, total = fc.indicator(Z, p=1.5)
        want = np.zeros_like(eta2)
        for e in range(fc.n_elements):
            for f in range(fc.n_local_faces):
                if ef[e, f] >= 0:
                    want[e] = want[e] + (0.5 * hF[ef[e, f]]) * J[ef[e, f]]
        assert np.array_equal(_bits(eta2), _bits(want)) and np.all(eta2[(ef >= 0).any(axis=1)] > 0)
        for c in range(3):
            ref = math.fsum(eta2[:, c])
            assert abs(total[c] - ref) <= 2 * EPS * abs(ref)
        e1, t1 = fc.indicator(Z[:, 1], p=1.5)
        assert isinstance(t1, float) and _bits(t1) == _bits(total[1]) and np.array_equal(_bits(e1), _bits(eta2[:, 1]))
        e2, t2 = m.jump_indicator(geom, Z, p=1.5, order=order)
        assert np.array_equal(_bits(e2), _bits(eta2)) and np.array_equal(_bits(t2), _bits(total))
        ims = fc.interior_measures()
        if geom.x.shape[2] == 2:                    # h_F = |F|: the sum of the face's measures in point order
            acc = np.zeros(len(ims))
            for q in range(ims.shape[1]):
                acc = acc + ims[:, q]
            assert np.array_equal(_bits(acc), _bits(hF))


def test_results_are_reproducible_and_independent_of_company():
    fn, order = cases.WARPED["fem2d_P2"]
    geom = fn()
    Z = cases.broken_field(geom, ncol=5)                                   # one more column than a chunk
    rng = np.random.default_rng(11)
    with m.Faces(geom) as fc:
        assert Z.shape[1] == fc.plan(1)["chunk"] + 1
        W = rng.standard_normal((fc.n_boundary, fc.n_points))
        for kind, p in [("value", 2.0), ("flux", 1.5), ("flux", 2.0)]:
            t1, f1 = fc.integrate(Z, kind=kind, p=p, weight=W, per_face=True)
            t2, f2 = fc.integrate(Z, kind=kind, p=p, weight=W, per_face=True)
            t3 = fc.integrate(Z, kind=kind, p=p, weight=W)
            assert np.array_equal(_bits(t1), _bits(t2)) and np.array_equal(_bits(f1), _bits(f2))     # run to run
            assert np.array_equal(_bits(t1), _bits(t3))                                              # per_face or not
            j1, j2 = fc.jumps(Z, kind=kind, p=p), fc.jumps(Z, kind=kind, p=p)
            assert np.array_equal(_bits(j1), _bits(j2))
            for c in range(Z.shape[1]):
                tc, fcol = fc.integrate(Z[:, c], kind=kind, p=p, weight=W, per_face=True)
                assert isinstance(tc, float) and _bits(tc) == _bits(t1[c]) and np.array_equal(_bits(fcol), _bits(f1[:, c]))
                assert np.array_equal(_bits(fc.jumps(Z[:, c], kind=kind, p=p)), _bits(j1[:, c]))
            # a face does not depend on the weight rows of other faces
            W2 = W.copy()
            keep = [1, fc.n_boundary - 2]
            W2[[b for b in range(fc.n_boundary) if b not in keep]] *= -3.0
            _, f4 = fc.integrate(Z, kind=kind, p=p, weight=W2, per_face=True)
            assert np.array_equal(_bits(f4[keep]), _bits(f1[keep])) and not np.array_equal(_bits(f4), _bits(f1))
        one = m.boundary_flux(geom, Z, p=1.5, weight=W)
        assert np.array_equal(_bits(one), _bits(fc.integrate(Z, kind="flux", p=1.5, weight=W)))


def test_lifecycle():
    geom = m.fem2d_P1()
    z = np.arange(6.0)
    fc = m.Faces(geom)
    v = fc.integrate(z)
    assert fc.last_times()["topology_ms"] > 0
    fc.close()
    fc.close()
    for call in (lambda: fc.integrate(z), lambda: fc.jumps(z), lambda: fc.indicator(z), fc.points, fc.normals, fc.measures,
                 fc.interior_measures, fc.face_sizes, fc.boundary_nodes, fc.last_times):
        with pytest.raises(ValueError, match="Faces: the faces are closed"):
            call()
    with m.Faces(geom) as f2:
        t = f2.last_times()
        assert t["face_ms"] == 0.0 and t["reduce_ms"] == 0.0 and t["topology_ms"] > 0
        assert _bits(f2.integrate(z)) == _bits(v)
        t = f2.last_times()
        assert t["face_ms"] > 0 and t["reduce_ms"] > 0
        assert f2.n_boundary == 4 and f2.n_interior == 1 and f2.jumps(z).shape == (1,)
        with pytest.raises(ValueError, match="weight must be \\(4, 3\\)"):
            f2.integrate(z, weight=np.ones((5, 3)))
        with pytest.raises(ValueError, match="kind must be"):
            f2.jumps(z, kind="energy")
    assert f2.closed
    with pytest.raises(ValueError, match="the faces are closed"):
        f2.integrate(z)
    with pytest.raises(ValueError, match="z has 5"):            # checked before the device is asked anything
        with m.Faces(geom) as f3:
            f3.integrate(np.zeros(5))
    one = m.fem2d(k=1)                                          # a single element: no interior faces
    with m.Faces(one) as f4:
        assert f4.n_interior == 0 and f4.jumps(np.zeros(4)).shape == (0,)
        eta2, total = f4.indicator(np.arange(4.0))
        assert total == 0.0 and np.array_equal(eta2, np.zeros(1))
