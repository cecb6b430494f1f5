"""A NumPy / SciPy restatement of `weld()` by a different algorithm, which the device is compared against.

The device sorts the corners into a grid and labels components by hooking and shortcutting (csrc/weld.hip).  Here the link
predicate is evaluated by brute force over all corner pairs, in blocks, and the classes come from
`scipy.sparse.csgraph.connected_components`; both are then renumbered by lowest member.  The semantics are fixed so that
the two give the same integers:

- corners `a`, `b` are linked iff their simplices have the same group and `fabs(x_a - x_b) <= tol` on every axis (one IEEE
  subtraction and one compare per axis);
- a vertex is a connected component of the link graph, numbered by its lowest corner (`first_corner`);
- the component of a vertex is its connected component in the graph of the simplex edges, numbered by lowest vertex;
- the normal of a vertex is the sum of `cross3(p1 - p0, p2 - p0)` over its corners in ascending corner order, divided by
  `sqrt((nx*nx + ny*ny) + nz*nz)`, zeros when that root is 0 or not finite.

The pair predicate is M^2 work: keep M at a few thousand corners.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components


@dataclass
class TwinMesh:
    vertices: np.ndarray
    cells: np.ndarray
    first_corner: np.ndarray
    component: np.ndarray
    ncomponents: int
    normals: Optional[np.ndarray]
    normal_bound: Optional[np.ndarray]   # (V,): sum |n_f| / |sum n_f| per vertex (inf where the normal is zero)
    vertex_data: Optional[np.ndarray]
    tol: float


def default_tol(points) -> float:
    P = np.asarray(points, dtype=np.float64)
    flat = P.reshape(-1, P.shape[-1])
    return 2.0 ** -27 * float(np.max(flat.max(axis=0) - flat.min(axis=0)))


def _by_lowest(n, rows, cols):
    """Labels of the components of the undirected graph on n nodes, renumbered by lowest member; (labels, lowest)."""
    A = sp.coo_matrix((np.ones(len(rows), dtype=np.int8), (rows, cols)), shape=(n, n)).tocsr()
    _, lab = connected_components(A, directed=False)
    lowest = np.full(lab.max() + 1 if n else 0, n, dtype=np.int64)
    np.minimum.at(lowest, lab, np.arange(n))
    order = np.argsort(lowest)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[lab].astype(np.int32), lowest[order].astype(np.int32)


def weld_twin(points, tol=None, normals=False, group=None, data=None, block=512) -> TwinMesh:
    P = np.ascontiguousarray(points, dtype=np.float64)
    S, nv, e = P.shape
    M = S * nv
    X = P.reshape(M, e)
    if tol is None:
        tol = default_tol(P)
    G = np.zeros(S, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    gc = np.repeat(G, nv)

    rows, cols = [], []
    for i0 in range(0, M, block):
        for j0 in range(0, M, block):
            near = np.abs(X[i0:i0 + block, None, :] - X[None, j0:j0 + block, :]).max(-1) <= tol
            near &= gc[i0:i0 + block, None] == gc[None, j0:j0 + block]
            i, j = np.nonzero(near)
            rows.append(i + i0)
            cols.append(j + j0)
    vid, first = _by_lowest(M, np.concatenate(rows), np.concatenate(cols))
    cells = vid.reshape(S, nv)
    V = first.size

    a = np.concatenate([cells[:, q] for q in range(nv)])
    b = np.concatenate([cells[:, (q + 1) % nv] for q in range(nv)])
    comp, lowest = _by_lowest(V, a, b)

    nrm = bound = None
    if normals:
        assert (nv, e) == (3, 3)
        nrm = np.zeros((V, 3))
        mag = np.zeros(V)
        for c in range(M):                     # ascending corner order, the operation order of cross3
            p0, p1, p2 = P[c // 3]
            u, w = p1 - p0, p2 - p0
            f = np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]])
            nrm[vid[c]] += f
            mag[vid[c]] += np.sqrt((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            ln = np.sqrt((nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1]) + nrm[:, 2] * nrm[:, 2])
            ok = (ln > 0) & np.isfinite(ln)
            bound = np.where(ok, mag / np.where(ok, ln, 1.0), np.inf)
            nrm = np.where(ok[:, None], nrm / np.where(ok, ln, 1.0)[:, None], 0.0)

    vdata = None
    if data is not None:
        D = np.asarray(data, dtype=np.float64)
        vdata = D.reshape(M, -1)[first]
    return TwinMesh(X[first], cells, first, comp, int(lowest.size), nrm, bound, vdata, float(tol))
