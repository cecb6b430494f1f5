"""Time `ClosestPointLocator` on the device: 1 M points within 0.01 of the cubed sphere m = 32, k = 2 (6,144 elements).

Prints one JSON line: wall-clock seconds to build the locator (uploads, location grid, points sorted by cell, every
candidate projected, nothing copied back) and the median seconds per `evaluate` over --reps warm calls (one upload of z,
the evaluation kernel, the copy back), with --gradient for values and tangential gradients.  A second line gives the
same two figures for a flat `PointLocator` on a `fem2d` k = 2 mesh of comparable size (L = 7: 4,096 elements) with the
same number of points, as context: that one inverts one element map per point, this one minimises a distance over every
candidate of the point's cell.  There is no pass / fail threshold.  Kernel durations come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/closest_bench.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402
from mgb_amd.tensorfem import _tf_nodes  # noqa: E402


def cubed_sphere(mm, k):
    """(p, 6 mm^2, 3): every face of [-1, 1]^3 cut into mm x mm Q_k quads, all tensor nodes projected onto the unit sphere."""
    nodes = np.array([-1.0, 1.0]) if k == 1 else _tf_nodes(k)
    h = 2.0 / mm
    c = -1.0 + h * np.arange(mm)
    u = c[None, :, None, None] + 0.5 * (nodes[None, None, None, :] + 1.0) * h       # (jj, ii, j, i) -> varies with ii, i
    v = c[:, None, None, None] + 0.5 * (nodes[None, None, :, None] + 1.0) * h       # ... with jj, j
    u, v = np.broadcast_arrays(u, v)
    faces = []
    for axis in range(3):
        a, b = [ax for ax in range(3) if ax != axis]
        for sign in (-1.0, 1.0):
            q = np.empty(u.shape + (3,))
            q[..., axis], q[..., a], q[..., b] = sign, u, v
            q /= np.sqrt((q * q).sum(axis=-1, keepdims=True))
            faces.append(q.reshape(mm * mm, len(nodes) ** 2, 3))
    return np.concatenate(faces, axis=0).transpose(1, 0, 2).copy()


def timed(make, evaluate, reps):
    t0 = time.perf_counter()
    loc = make()
    create = time.perf_counter() - t0
    try:
        evaluate(loc)                                  # warm-up: code objects of the evaluate kernel, result buffers
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = evaluate(loc)
            times.append(time.perf_counter() - t0)
    finally:
        loc.close()
    return create, float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--points", type=int, default=2 ** 20)
    ap.add_argument("--offset", type=float, default=0.01)
    ap.add_argument("--L", type=int, default=7, help="subdivision level of the flat fem2d mesh of the second line")
    ap.add_argument("--gradient", action="store_true", help="also evaluate the tangential gradient at every foot")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    M = args.points

    geom = m.fem2d(k=args.k, K=cubed_sphere(args.m, args.k), ambient=3)
    dirs = rng.standard_normal((M, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    pts = dirs * (1.0 + rng.uniform(-args.offset, args.offset, size=(M, 1)))
    a = rng.standard_normal(3)
    z = geom.xflat @ a + 0.5
    m.ClosestPointLocator(geom, pts[:256]).close()     # warm-up: context, code objects of the build
    ev = (lambda loc: loc.evaluate(z, gradient=True)) if args.gradient else (lambda loc: (loc.evaluate(z), None))
    keep = {}

    def make():
        keep["cp"] = m.ClosestPointLocator(geom, pts)
        return keep["cp"]
    create, per, (vals, _) = timed(make, ev, args.reps)
    # the affine field is reproduced at the foot, which lies within O(h^3) of the point's radial projection
    print(json.dumps(dict(case=f"cubed sphere m={args.m} k={args.k}", elements=int(geom.x.shape[1]), points=M,
                          gradient=args.gradient, max_distance=keep["cp"].max_distance, seconds_create=create,
                          seconds_per_evaluate=per, without_foot=int(np.isnan(vals).sum()),
                          max_err_against_radial_projection=float(np.nanmax(np.abs(vals - (dirs @ a + 0.5)))))), flush=True)

    flat = m.subdivide(m.fem2d(k=2), args.L)
    fpts = rng.uniform(-1, 1, (M, 2))
    b = rng.standard_normal(2)
    fz = flat.xflat @ b + 0.5
    m.PointLocator(flat, fpts[:256]).close()
    fev = (lambda loc: loc.evaluate(fz, gradient=True)) if args.gradient else (lambda loc: (loc.evaluate(fz), None))
    create, per, (fvals, _) = timed(lambda: m.PointLocator(flat, fpts), fev, args.reps)
    print(json.dumps(dict(case=f"flat fem2d k=2 L={args.L} (PointLocator)", elements=int(flat.x.shape[1]), points=M,
                          gradient=args.gradient, seconds_create=create, seconds_per_evaluate=per,
                          max_err=float(np.nanmax(np.abs(fvals - (fpts @ b + 0.5)))))), flush=True)


if __name__ == "__main__":
    main()
