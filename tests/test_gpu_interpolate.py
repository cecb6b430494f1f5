"""interpolate() on the device (-m gpu): reproduction of functions in the element space, the reference's 1-D and
spectral semantics against a NumPy transcription, nested meshes, real solves, scale and determinism."""
import zlib

import numpy as np
import pytest

import mgb_amd as m
from helpers import record_observation
from mgb_amd.spectral import _chebyshev_values, evaluation
from mgb_amd.tensorfem import _tf_nodes

pytestmark = pytest.mark.gpu

REPRO_RTOL = 1e-12
REF_TOL = 1e-13


def _relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _poly(rng, d, k):
    """A random polynomial of degree k in each of d variables, vectorised over (M, d) points."""
    C = rng.standard_normal((k + 1,) * d)

    def f(X):
        X = np.atleast_2d(X)
        out = np.zeros(X.shape[0])
        for idx in np.ndindex(*C.shape):
            term = np.full(X.shape[0], C[idx])
            for a, e in enumerate(idx):
                term = term * X[:, a] ** e
            out += term
        return out
    return f


def _interior(rng, M, d, margin=1e-3):
    return rng.uniform(-1 + margin, 1 - margin, size=(M, d))


# ---------------------------------------------------------------------------------------------------------------------
# 1. reproduction
# ---------------------------------------------------------------------------------------------------------------------

REPRO = ([("fem1d", k) for k in (1, 2, 3, 4)] + [("fem2d", k) for k in (1, 2, 3)] + [("fem3d", k) for k in (1, 2, 3)]
         + [("fem2d_P1", 1), ("fem2d_P2", 2), ("fem2d_P2_nobubble", 2)]
         + [("spectral1d", 4), ("spectral1d", 16), ("spectral2d", 4), ("spectral2d", 16)])


def _repro_geom(name, k):
    if name == "fem1d":
        return m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 4), k=k), 4), 1, k
    if name == "fem2d":
        return m.subdivide(m.fem2d(k=k), 3), 2, k
    if name == "fem3d":
        return m.subdivide(m.fem3d(k=k), 2), 3, k
    if name == "fem2d_P1":
        return m.subdivide(m.fem2d_P1(), 4), 2, 1
    if name == "fem2d_P2":
        return m.subdivide(m.fem2d_P2(), 4), 2, 2
    if name == "fem2d_P2_nobubble":
        return m.subdivide(m.fem2d_P2(bubble=False), 4), 2, 2
    if name == "spectral1d":
        return m.spectral1d(n=k), 1, k - 1
    return m.spectral2d(n=k), 2, k - 1


@pytest.mark.parametrize("name,k", REPRO)
def test_reproduces_functions_of_the_element_space(name, k):
    rng = np.random.default_rng(zlib.crc32(f"{name}{k}".encode()))
    geom, d, deg = _repro_geom(name, k)
    if name in ("fem2d_P1", "fem2d_P2", "fem2d_P2_nobubble"):      # total degree: linear / quadratic
        a = rng.standard_normal(6)
        f = lambda X: (a[0] + a[1] * X[:, 0] + a[2] * X[:, 1]
                       + (a[3] * X[:, 0] ** 2 + a[4] * X[:, 0] * X[:, 1] + a[5] * X[:, 1] ** 2 if deg == 2 else 0))
    else:
        f = _poly(rng, d, deg)
    z = f(geom.xflat)
    pts = _interior(rng, 100_000, d)
    vals = m.interpolate(geom, z, pts[:, 0] if d == 1 else pts)
    err = _relerr(vals, f(pts))
    record_observation(f"interpolate reproduction {name} k={k}: max rel err {err:.3e}")
    assert np.all(np.isfinite(vals)) and err <= REPRO_RTOL, err


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference's 1-D and spectral semantics (NumPy transcription of src/TensorFEM.jl:967-1014,
#    src/spectral1d.jl:140-170, src/spectral2d.jl:85-125)
# ---------------------------------------------------------------------------------------------------------------------

def _lagrange(nodes, xv):
    s = len(nodes)
    out = []
    for i in range(s):
        num = den = 1.0
        for j in range(s):
            if i != j:
                num *= xv - nodes[j]
                den *= nodes[i] - nodes[j]
        out.append(num / den)
    return out


def ref_fem1d(geom, z, tq):
    x = geom.x[:, :, 0]                      # (s, N)
    s, N = x.shape
    nodes1 = _tf_nodes(geom.discretization.k)
    lefts = x[0]
    srt = bool(np.all(lefts[1:] >= lefts[:-1]))
    x_lo, x_hi = x[0, 0], x[s - 1, N - 1]
    tq = float(tq)
    if tq <= x_lo:
        return z[0]
    if tq >= x_hi:
        return z[s * N - 1]
    if srt:
        e = min(max(int(np.searchsorted(lefts, tq, side="right")) - 1, 0), N - 1)
    else:
        e = 0
        while e < N - 1 and tq > x[s - 1, e]:
            e += 1
    lo, hi = -1.0, 1.0
    flo = float(x[0, e]) - tq
    if flo == 0.0:
        return z[e * s]
    fhi = float(x[s - 1, e]) - tq
    if fhi == 0.0:
        return z[e * s + s - 1]
    xi = 0.0
    for _ in range(128):
        xi = (lo + hi) / 2
        if xi == lo or xi == hi:
            break
        L = _lagrange(nodes1, xi)
        fmid = 0.0
        for j in range(s):
            fmid += L[j] * float(x[j, e])
        fmid -= tq
        if fmid == 0.0:
            break
        if np.signbit(fmid) == np.signbit(flo):
            lo, flo = xi, fmid
        else:
            hi = xi
    L = _lagrange(nodes1, xi)
    v = 0.0
    for j in range(s):
        v += L[j] * float(z[e * s + j])
    return v


def ref_spectral1d(geom, z, tq):
    x = geom.xflat[:, 0]
    c = np.linalg.solve(evaluation(x, len(x)), z)
    return float(c @ _chebyshev_values(float(tq), len(c)))


def ref_spectral2d(geom, z, pt):
    n = geom.discretization.n
    V = evaluation(geom.xflat[:n, 0], n)
    C = np.linalg.solve(V, np.linalg.solve(V, z.reshape(n, n, order="F")).T).T      # V \ Z / V'
    bx, by = _chebyshev_values(float(pt[0]), n), _chebyshev_values(float(pt[1]), n)
    return float(bx @ (C @ by))


def _fem1d_cases():
    sub = m.subdivide(m.fem1d(nodes=np.linspace(-1, 1, 3), k=3), 3)
    rng = np.random.default_rng(11)
    nodes = np.sort(np.concatenate([[-1.0, 1.0], rng.uniform(-1, 1, 9)]))
    K = np.stack([nodes[:-1], nodes[1:]])[:, :, None]
    perm = rng.permutation(K.shape[1])
    unsorted = m.fem1d(K=K[:, perm, :], k=2)
    assert not np.all(np.diff(unsorted.x[0, :, 0]) >= 0)
    return [("k1", m.fem1d(nodes=np.linspace(-1, 1, 9))), ("k3_subdivided", sub),
            ("k4", m.fem1d(nodes=nodes, k=4)), ("k2_unsorted", unsorted)]


@pytest.mark.parametrize("label,geom", _fem1d_cases())
def test_fem1d_is_the_reference_algorithm(label, geom):
    rng = np.random.default_rng(5)
    z = rng.standard_normal(geom.xflat.shape[0])
    xs = geom.xflat[:, 0]
    inside = rng.uniform(-1, 1, 400)
    outside = np.array([-3.0, -1.0 - 1e-15, -1.0, 1.0, 1.0 + 1e-15, 2.5, np.inf, -np.inf])
    lefts = geom.x[0, :, 0]
    pts = np.concatenate([inside, outside, xs, lefts])
    dev = m.interpolate(geom, z, pts)
    ref = np.array([ref_fem1d(geom, z, t) for t in pts])
    err = float(np.abs(dev - ref).max() / np.abs(z).max())
    record_observation(f"interpolate fem1d {label} vs reference transcription: max err {err:.3e}")
    assert err <= REF_TOL
    nodes_part = slice(len(inside) + len(outside), None)
    assert np.array_equal(dev[nodes_part], ref[nodes_part])        # exact nodes and shared interior nodes
    assert np.array_equal(dev[len(inside):len(inside) + len(outside)], ref[len(inside):len(inside) + len(outside)])
    # scalar in, scalar out; array shape kept
    assert isinstance(m.interpolate(geom, z, 0.25), float)
    assert m.interpolate(geom, z, inside[:6].reshape(2, 3)).shape == (2, 3)
    assert np.isnan(m.interpolate(geom, z, np.nan))


@pytest.mark.parametrize("n", [4, 7, 16])
def test_spectral_is_the_reference_formula(n):
    rng = np.random.default_rng(n)
    g1 = m.spectral1d(n=n)
    z1 = rng.standard_normal(n)
    t = np.concatenate([rng.uniform(-1, 1, 300), [-1.0, 1.0, -1.3, 1.7], g1.xflat[:, 0]])
    dev1 = m.interpolate(g1, z1, t)
    ref1 = np.array([ref_spectral1d(g1, z1, tt) for tt in t])
    g2 = m.spectral2d(n=n)
    z2 = rng.standard_normal(g2.xflat.shape[0])
    P = np.concatenate([rng.uniform(-1, 1, (300, 2)), [[-1.2, 0.3], [1.0, 1.0]], g2.xflat])
    dev2 = m.interpolate(g2, z2, P)
    ref2 = np.array([ref_spectral2d(g2, z2, p) for p in P])
    e1 = float(np.abs(dev1 - ref1).max() / np.abs(ref1).max())
    e2 = float(np.abs(dev2 - ref2).max() / np.abs(ref2).max())
    record_observation(f"interpolate spectral n={n} vs reference transcription: 1-D {e1:.3e}, 2-D {e2:.3e}")
    assert e1 <= REF_TOL and e2 <= REF_TOL
    assert isinstance(m.interpolate(g2, z2, np.array([0.1, 0.2])), float)


def test_reference_docstring_examples():
    geom = m.subdivide(m.fem1d(nodes=np.linspace(-1.0, 1.0, 3)), 3)
    z = np.sin(np.pi * geom.xflat[:, 0])
    y = m.interpolate(geom, z, 0.5)
    y_vec = m.interpolate(geom, z, [-0.5, 0.0, 0.5])
    assert y == ref_fem1d(geom, z, 0.5)
    assert np.array_equal(y_vec, [ref_fem1d(geom, z, t) for t in (-0.5, 0.0, 0.5)])
    g2 = m.spectral2d(n=4)
    xf = g2.xflat
    z2 = np.exp(-xf[:, 0] ** 2 - xf[:, 1] ** 2)
    points = np.array([[0.0, 0.0], [0.5, 0.5], [-0.5, 0.5]])
    vals = m.interpolate(g2, z2, points)
    ref = np.array([ref_spectral2d(g2, z2, p) for p in points])
    record_observation(f"interpolate docstring examples: fem1d {abs(y - ref_fem1d(geom, z, 0.5)):.1e}, "
                       f"spectral2d {np.abs(vals - ref).max():.3e}")
    assert vals.shape == (3,) and np.abs(vals - ref).max() <= REF_TOL


# ---------------------------------------------------------------------------------------------------------------------
# 3. nested meshes: a level-l function lifted to levels L-1 and L by the geometric hierarchies
# ---------------------------------------------------------------------------------------------------------------------

NESTED = [("fem2d_P1", lambda: m.fem2d_P1(), 4), ("fem2d_P2", lambda: m.fem2d_P2(bubble=False), 4),
          ("fem2d_Q2", lambda: m.fem2d(k=2), 3), ("fem3d_Q2", lambda: m.fem3d(k=2), 3)]


@pytest.mark.parametrize("name,make,L", NESTED)
def test_coarse_lift_interpolates_to_the_fine_lift(name, make, L):
    """A random continuous function of level l = L - 2 (one value per mesh node, boundary included), as coefficients
    of that level's `:full` space, lifted by geometric_mg(g0, L - 1) and geometric_mg(g0, L): interpolating the coarse
    lift at the fine nodes gives the fine lift (both hierarchies number level l alike: tests/test_interpolate.py)."""
    g0 = make()
    coarse, fine = m.geometric_mg(g0, L - 1), m.geometric_mg(g0, L)
    lvl = L - 2
    Rc, Rf = coarse.R["full"][lvl], fine.R["full"][lvl]
    labels = m.subdivide(g0, lvl + 1).labels
    rng = np.random.default_rng(L)
    c = rng.standard_normal(labels.max() + 1)[labels]            # continuous: shared nodes share a value
    zc, zf = Rc @ c, Rf @ c
    gc, gf = m.subdivide(g0, L - 1), m.subdivide(g0, L)
    vals, elem = m.interpolate(gc, zc, gf.xflat, return_element=True)
    err = _relerr(vals, zf)
    record_observation(f"interpolate nested {name} L={L - 1}->{L} (:full, continuous): max rel err {err:.3e}")
    assert np.all(elem >= 0) and err <= REPRO_RTOL, err


# ---------------------------------------------------------------------------------------------------------------------
# 4. real solves
# ---------------------------------------------------------------------------------------------------------------------

def test_solution_at_its_own_nodes_fem2d_P2():
    geom = m.subdivide(m.fem2d_P2(), 4)
    sol = m.mgb_solve(m.assemble(m.amg(geom), p=1.5))
    z = sol.z[:, 0]
    vals = m.interpolate(geom, z, geom.xflat)
    err = _relerr(vals, z)
    record_observation(f"interpolate fem2d_P2 L=4 solve at its nodes: max rel err {err:.3e}")
    assert err <= REPRO_RTOL, err


def test_solution_at_its_own_nodes_zoo_p_harmonic_3d():
    """Columns u1..u3 are continuous and come back at every node; the slack s lives in the broken space, so at a node
    shared by several elements it comes back as the value of the element that was used (the lowest-index one)."""
    geom = m.subdivide(m.fem3d(k=2), 2)
    sol = m.mgb_solve(m.Zoo.p_harmonic(m.amg(geom)))
    Z = sol.z
    allcols, elem = m.interpolate(geom, Z, geom.xflat, return_element=True)
    p = geom.x.shape[0]
    X = geom.xflat.reshape(-1, p, 3)
    local = np.abs(X[elem] - geom.xflat[:, None, :]).max(axis=2).argmin(axis=1)
    rows = elem.astype(np.int64) * p + local
    errs = []
    for j in range(Z.shape[1]):
        col = m.interpolate(geom, Z[:, j], geom.xflat)
        assert np.array_equal(col, allcols[:, j])
        errs.append(_relerr(col, Z[rows, j]))
        if j < 3:
            errs.append(_relerr(col, Z[:, j]))
    record_observation("interpolate fem3d Zoo p_harmonic at its nodes: max rel err per check "
                       + ", ".join(f"{e:.3e}" for e in errs))
    assert max(errs) <= REPRO_RTOL, errs


# ---------------------------------------------------------------------------------------------------------------------
# 5. scale and determinism
# ---------------------------------------------------------------------------------------------------------------------

def test_scale_outside_nan_and_determinism():
    geom = m.subdivide(m.fem2d_P2(), 8)
    rng = np.random.default_rng(8)
    a = rng.standard_normal(6)
    f = lambda X: a[0] + a[1] * X[:, 0] + a[2] * X[:, 1] + a[3] * X[:, 0] ** 2 + a[4] * X[:, 0] * X[:, 1] + a[5] * X[:, 1] ** 2
    pts = rng.uniform(-1, 1, (2_000_000, 2))
    z = f(geom.xflat)
    vals, elem = m.interpolate(geom, z, pts, return_element=True)
    err = _relerr(vals, f(pts))
    record_observation(f"interpolate fem2d_P2 L=8, 2M points: max rel err {err:.3e}")
    assert np.all(elem >= 0) and err <= REPRO_RTOL, err
    bad = np.array([[1.5, 0.0], [0.0, -1.0 - 1e-6], [3.0, 3.0], [np.nan, 0.0], [0.0, np.nan], [np.inf, 0.0],
                    [-np.inf, np.inf]])
    bv, be = m.interpolate(geom, z, bad, return_element=True)
    assert np.all(np.isnan(bv)) and np.all(be == -1)
    assert np.isnan(m.interpolate(geom, z, np.array([2.0, 2.0])))
    again, elem2 = m.interpolate(geom, z, pts, return_element=True)
    assert np.array_equal(again, vals) and np.array_equal(elem2, elem)
    Z = np.stack([z, np.cos(geom.xflat[:, 0]), -2 * z], axis=1)
    sub = pts[:200_000]
    multi = m.interpolate(geom, Z, sub)
    assert multi.shape == (sub.shape[0], 3)
    for j in range(3):
        assert np.array_equal(multi[:, j], m.interpolate(geom, Z[:, j], sub))


def test_shared_faces_take_the_lowest_element():
    geom = m.subdivide(m.fem2d_P1(), 3)
    z = np.arange(geom.xflat.shape[0], dtype=np.float64)        # discontinuous: the element is visible in the value
    vals, elem = m.interpolate(geom, z, geom.xflat, return_element=True)
    # every node lies in the elements that share it; the lowest index wins
    X = geom.xflat.reshape(-1, 3, 2)
    for q in range(0, geom.xflat.shape[0], 7):
        pt = geom.xflat[q]
        owners = [e for e in range(X.shape[0]) if np.any(np.all(np.abs(X[e] - pt) <= 1e-14, axis=1))]
        assert elem[q] == min(owners)
    assert m.interpolate(geom, z, np.zeros((0, 2))).shape == (0,)


# ---------------------------------------------------------------------------------------------------------------------
# 6. meshes far from the origin and fine meshes: the Newton and containment tolerances follow the rounding level
# ---------------------------------------------------------------------------------------------------------------------

SHIFTED = [("fem2d_Q1_at_1000", lambda: m.fem2d(k=1, K=m.fem2d(k=1).x + 1000.0), 5, 1000.0, 1),
           ("fem2d_Q2_at_100", lambda: m.fem2d(k=2, K=m.fem2d(k=2).x + 100.0), 7, 100.0, 2),
           ("fem3d_Q1_at_1000", lambda: m.fem3d(k=1, K=m.fem3d(k=1).x + 1000.0), 4, 1000.0, 1),
           ("fem2d_P1_at_1000", lambda: m.fem2d_P1(K=m.fem2d_P1().x + 1000.0), 8, 1000.0, 1),
           ("fem2d_P2_at_1000", lambda: m.fem2d_P2(K=m.fem2d_P2().x + 1000.0), 7, 1000.0, 2)]


@pytest.mark.parametrize("name,make,L,shift,deg", SHIFTED)
def test_translated_meshes_find_every_point(name, make, L, shift, deg):
    geom = m.subdivide(make(), L)
    d = geom.x.shape[2]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    a = rng.standard_normal(3)
    f = lambda X: a[0] + a[1] * (X[:, 0] - shift) + a[2] * (X[:, d - 1] - shift) ** deg
    z = f(geom.xflat)
    pts = np.concatenate([shift + _interior(rng, 200_000, d, margin=0.0), geom.xflat])   # random points and every node
    vals, elem = m.interpolate(geom, z, pts, return_element=True)
    missing = int(np.count_nonzero(elem < 0))
    err = _relerr(vals, f(pts)) if missing == 0 else float("nan")
    record_observation(f"interpolate translated {name} L={L}: {missing} points not found, max rel err {err:.3e}")
    assert missing == 0 and np.all(np.isfinite(vals))
    assert err <= 1e-10, err


def test_fine_q1_mesh_finds_every_point():
    geom = m.subdivide(m.fem2d(k=1), 11)                           # 1024 x 1024 elements
    rng = np.random.default_rng(1024)
    a = rng.standard_normal(4)
    f = lambda X: a[0] + a[1] * X[:, 0] + a[2] * X[:, 1] + a[3] * X[:, 0] * X[:, 1]
    z = f(geom.xflat)
    pts = _interior(rng, 2_000_000, 2, margin=0.0)
    vals, elem = m.interpolate(geom, z, pts, return_element=True)
    missing = int(np.count_nonzero(elem < 0))
    err = _relerr(vals, f(pts)) if missing == 0 else float("nan")
    record_observation(f"interpolate fem2d Q1 L=11, 2M points: {missing} not found, max rel err {err:.3e}")
    assert missing == 0 and err <= REPRO_RTOL, err
