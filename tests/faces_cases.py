"""The meshes and fields the face tests share (tests/test_faces.py on the CPU, tests/test_gpu_faces.py on the device)."""
import dataclasses
import itertools

import numpy as np

import mgb_amd as m


def warp(x, amp=0.06):
    """A smooth map of the nodes (that of tests/test_gpu_integrate.py): elements stay valid and conforming, no element map
    stays affine."""
    y = x.copy()
    s = x.sum(axis=-1)
    for a in range(x.shape[-1]):
        y[..., a] += amp * np.sin(1.3 * s + 0.7 * a) + 0.5 * amp * x[..., (a + 1) % x.shape[-1]] ** 2
    return y


# ---- the meshes whose topology is compared with the twin -----------------------------------------------------------

def l_shape(k=1):
    """Three squares [-1, 0] x [-1, 0], [0, 1] x [-1, 0], [-1, 0] x [0, 1] given through K."""
    ref = m.fem2d(k=k).x[:, 0, :]                                   # the nodes of [-1, 1]^2
    cells = [(-0.5, -0.5), (0.5, -0.5), (-0.5, 0.5)]
    return m.fem2d(k=k, K=np.stack([0.5 * ref + np.array(c) for c in cells], axis=1))


def relabelled(geom, base=2 ** 21 + 5, stride=3):
    """The same mesh with its node ids mapped injectively above 2^21."""
    return dataclasses.replace(geom, t=base + stride * np.asarray(geom.t))


def three_on_an_edge():
    """Three quadrilaterals whose explicit `t` shares one edge (ids 0, 1) among all three."""
    ref = m.fem2d(k=1).x[:, 0, :]
    g = m.fem2d(k=1, K=np.stack([ref + np.array([3.0 * j, 0.0]) for j in range(3)], axis=1))
    t = np.array([[0, 1, 2, 3], [0, 1, 4, 5], [0, 1, 6, 7]]).T
    return dataclasses.replace(g, t=t)


TOPOLOGY = {
    "fem2d_k1": lambda: m.subdivide(m.fem2d(k=1), 2),
    "fem2d_k2": lambda: m.subdivide(m.fem2d(k=2), 2),
    "fem3d_k1": lambda: m.subdivide(m.fem3d(k=1), 2),
    "fem3d_k2": lambda: m.subdivide(m.fem3d(k=2), 2),
    "fem2d_P1": lambda: m.subdivide(m.fem2d_P1(), 2),
    "fem2d_P2": lambda: m.subdivide(m.fem2d_P2(), 2),
    "fem2d_P2_nobubble": lambda: m.subdivide(m.fem2d_P2(bubble=False), 2),
    "l_shape": l_shape,
    "fem3d_k1_relabelled": lambda: relabelled(m.subdivide(m.fem3d(k=1), 2)),
    "fem2d_P2_relabelled": lambda: relabelled(m.subdivide(m.fem2d_P2(), 2)),
}


# ---- every relative orientation of two elements ----------------------------------------------------------------------

def rotations(d):
    """The signed permutation matrices of determinant +1: 4 in 2-D, 24 in 3-D."""
    out = []
    for perm in itertools.permutations(range(d)):
        for signs in itertools.product((1.0, -1.0), repeat=d):
            R = np.zeros((d, d))
            for a in range(d):
                R[a, perm[a]] = signs[a]
            if np.linalg.det(R) > 0:
                out.append(R)
    return out


def pair(d, k, R):
    """Two elements: [-1, 1]^d and its neighbour across x = 1, whose local axes are those of the first turned by R."""
    make = m.fem2d if d == 2 else m.fem3d
    c = make(k=k).x[:, 0, :]
    shift = np.zeros(d)
    shift[0] = 2.0
    return make(k=k, K=np.stack([c, c @ R.T + shift], axis=1))


def polynomial(X, k):
    """A polynomial of the element space Q_k (so its sampled z is conforming and its flux continuous) that is symmetric
    along no face."""
    x, y = X[:, 0], X[:, 1]
    z = X[:, 2] if X.shape[1] == 3 else 0.0 * x
    u = 1.0 + x + 2.0 * y - 3.0 * z + 0.7 * x * y + 0.4 * y * z - 0.6 * x * z + 0.3 * x * y * z
    if k >= 2:
        u = u + 0.5 * x * x * y - 0.25 * y * y * z + 0.2 * z * z * x + 0.35 * y * y - 0.15 * z * z
    return u


# ---- warped meshes and fields --------------------------------------------------------------------------------------

WARPED = {
    "fem2d_k2": (lambda: m.fem2d(k=2, K=warp(m.subdivide(m.fem2d(k=2), 2).x)), None),
    "fem3d_k1": (lambda: m.fem3d(k=1, K=warp(m.subdivide(m.fem3d(k=1), 2).x, 0.03)), 4),    # Qf = 16: two workgroups of boundary faces
    "fem3d_k2": (lambda: m.fem3d(k=2, K=warp(pair(3, 2, np.eye(3)).x, 0.03)), 3),
    "fem2d_P1": (lambda: m.fem2d_P1(K=warp(m.subdivide(m.fem2d_P1(), 2).x)), None),
    "fem2d_P2": (lambda: m.fem2d_P2(K=warp(m.subdivide(m.fem2d_P2(), 2).x), curved=True), None),
    "fem2d_P2_nobubble": (lambda: m.fem2d_P2(bubble=False, K=warp(m.fem2d_P2(bubble=False).x), curved=True), None),
}


def broken_field(geom, ncol=2, seed=0):
    """Z (p N, ncol): a smooth function with a gradient well away from zero plus a small element-wise perturbation, so
    that both jumps are nonzero and no gradient drowns in its own rounding error."""
    X = geom.xflat
    rng = np.random.default_rng(seed + X.shape[0])
    x, y = X[:, 0], X[:, 1]
    base = 1.5 * x - 0.8 * y + 0.4 * np.sin(1.1 * x + 0.6 * y) + (0.9 * X[:, 2] if X.shape[1] == 3 else 0.0)
    return np.stack([base * (1 + 0.25 * c) + 0.02 * rng.standard_normal(X.shape[0]) + 0.1 * c for c in range(ncol)], axis=1)
