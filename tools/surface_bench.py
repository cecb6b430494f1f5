"""Time the reference's default figure on the device: fem3d (k = 3) at L = 5, the five default isosurfaces, an
800 x 600 pinhole image.

Prints one JSON line: the number of triangles, wall-clock seconds to build the triangle caster (upload, boxes, count,
scan, emit, sort; after one small warm-up caster that loads the code objects), the median wall-clock seconds per `trace`
and per `shade` over --reps warm calls, and per frame of `RayCaster.render(u, layers=...)` on a caster built once (upload
of u and the layers, evaluation, compositing, copy back), the share of rays that hit and the mean alpha as a checksum.
Kernel durations come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/surface_bench.py`.
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
from mgb_amd.raycast import clip_box, default_transfer  # noqa: E402
from mgb_amd.surface import REFERENCE_ISOSURFACES  # noqa: E402

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


def smooth(X):
    return np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1] - 0.2) + 0.35 * np.sin(1.1 * X[:, 2] + 0.3)


def median_seconds(f, reps):
    f()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    args = ap.parse_args()
    geom = m.subdivide(m.fem3d(k=args.k), args.L)
    u = smooth(geom.xflat)
    lo, hi = float(u.min()), float(u.max())
    levels = np.array(REFERENCE_ISOSURFACES) * (hi - lo) + lo
    box = clip_box(geom)
    diagonal = float(np.linalg.norm(box[1] - box[0]))
    step = diagonal / 256.0
    table = default_transfer(diagonal)
    opaque = table.copy()
    opaque[:, 3] = 1.0
    o, d = m.camera_rays(EYE, TARGET, size=(args.width, args.height), fov=30.0)
    soup = m.isocontour(geom, u, levels)
    values = np.repeat(levels[soup.level][:, None], 3, axis=1)
    with m.TriangleCaster(soup.points[:64]) as warm:               # warm-up: context, code objects
        warm.trace(o[:64], d[:64])
    t0 = time.perf_counter()
    tc = m.TriangleCaster(soup.points)
    build = time.perf_counter() - t0
    with tc:
        trace, hits = median_seconds(lambda: tc.trace(o, d), args.reps)
        shade, layers = median_seconds(lambda: tc.shade(hits, d, values, opaque, (lo, hi)), args.reps)
    with m.RayCaster(geom, o, d, step) as rc:
        frame, rgba = median_seconds(lambda: rc.render(u, table, (lo, hi), layers=(hits.t, layers)), args.reps)
        plain, _ = median_seconds(lambda: rc.render(u, table, (lo, hi)), args.reps)
        samples = rc.nsamples
    res = dict(case=f"fem3d k={args.k} L={args.L} {args.width}x{args.height}, {len(levels)} isosurfaces",
               triangles=int(soup.points.shape[0]), rays=int(o.shape[0]), samples=samples, build_seconds=build,
               trace_seconds=trace, shade_seconds=shade, frame_seconds=frame, frame_seconds_without_layers=plain,
               rays_hit=float((hits.triangle[:, 0] >= 0).mean()), mean_alpha=float(rgba[:, 3].mean()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
