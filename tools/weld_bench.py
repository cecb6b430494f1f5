"""Time `weld` on the device: the five isosurfaces of fem3d (k = 3) at L = 5 and the five level curves of fem2d_P2 at
L = 9, default `refine`, default tolerance, with normals on the triangles.

Prints one JSON line per case: wall-clock seconds per call (median of --reps calls after one warm-up; the call includes
the upload of the soup, both sorts, every labelling round and the copy back), the corners, vertices and components, the
labelling rounds, and whether the mesh is closed.  With --host the line also carries the wall-clock of a NumPy weld of the
same soup (coordinates rounded to the tolerance and `np.unique`; classes that straddle a rounding boundary are not joined,
so its vertex count can differ): a NumPy figure for orientation, not a tuned CPU baseline.  Kernel durations come from a
run under `rocprofv3 --kernel-trace --stats -- python tools/weld_bench.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mgb_amd as m  # noqa: E402

LEVELS = np.array([-0.31, -0.12, 0.07, 0.23, 0.41])


def smooth(X):
    w = X[:, 2] if X.shape[1] == 3 else 0.0
    return np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1] - 0.2) + 0.35 * np.sin(1.1 * w + 0.3)


def numpy_weld(points, level, tol):
    """Vertices by rounding to a lattice of pitch 4 tol and `np.unique` over (level, lattice point)."""
    S, nv, e = points.shape
    q = np.round(points.reshape(-1, e) / (4.0 * tol)).astype(np.int64)
    key = np.concatenate([np.repeat(level.astype(np.int64), nv)[:, None], q], axis=1)
    _, first, inverse = np.unique(key, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first)
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[inverse.reshape(-1)].reshape(S, nv)


def run(name, geom, reps, host):
    c = m.isocontour(geom, smooth(geom.xflat), LEVELS)
    normals = c.points.shape[1:] == (3, 3)
    m.weld(c, normals=normals)                        # warm-up: context, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mesh = m.weld(c, normals=normals)
        times.append(time.perf_counter() - t0)
    res = dict(case=name, simplices=int(c.level.size), corners=int(c.points.shape[0] * c.points.shape[1]),
               vertices=int(mesh.vertices.shape[0]), components=int(mesh.ncomponents), rounds=list(mesh.rounds),
               tol=mesh.tol, closed=mesh.is_closed(), boundary_edges=int(mesh.boundary_edges().shape[0]),
               degenerate=int(mesh.degenerate().sum()), seconds_per_call=float(np.median(times)))
    if host:
        t0 = time.perf_counter()
        cells = numpy_weld(c.points, c.level, mesh.tol)
        res["numpy_weld_seconds"] = time.perf_counter() - t0
        res["numpy_weld_vertices"] = int(cells.max()) + 1
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2", type=int, default=9)
    ap.add_argument("--L3", type=int, default=5)
    ap.add_argument("--host", action="store_true", help="also time a NumPy weld of the same soup")
    args = ap.parse_args()
    run(f"fem3d k=3 L={args.L3}", m.subdivide(m.fem3d(k=3), args.L3), args.reps, args.host)
    run(f"fem2d_P2 L={args.L2}", m.subdivide(m.fem2d_P2(), args.L2), args.reps, args.host)


if __name__ == "__main__":
    main()
