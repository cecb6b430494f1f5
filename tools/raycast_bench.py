"""Time the volume render on the device: fem3d (k = 3) at L = 5, an 800 x 600 pinhole image, the default step
(1/256 of the clip box's diagonal), the default transfer table and clim.

Prints one JSON line: wall-clock seconds to build the caster (count, scan, emit, locate; after one small warm-up caster
that loads the code objects), the median wall-clock seconds per `render` over --reps warm calls (upload of u, evaluation,
compositing, copy back of the R x 4 result), the number of rays and samples, the bytes resident per sample and the mean
alpha as a checksum.  Kernel durations come from a run of its own under
`rocprofv3 --kernel-trace --stats -- python tools/raycast_bench.py`.
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
from mgb_amd.raycast import clip_box  # noqa: E402

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


def smooth(X):
    return np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1] - 0.2) + 0.35 * np.sin(1.1 * X[:, 2] + 0.3)


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
    box = clip_box(geom)
    step = float(np.linalg.norm(box[1] - box[0])) / 256.0
    o, d = m.camera_rays(EYE, TARGET, size=(args.width, args.height), fov=30.0)
    with m.RayCaster(geom, o[:64], d[:64], step) as warm:          # warm-up: context, code objects
        warm.render(u)
    t0 = time.perf_counter()
    rc = m.RayCaster(geom, o, d, step)
    build = time.perf_counter() - t0
    with rc:
        rc.render(u)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rgba = rc.render(u)
            times.append(time.perf_counter() - t0)
        res = dict(case=f"fem3d k={args.k} L={args.L} {args.width}x{args.height}", elements=int(geom.x.shape[1]),
                   rays=rc.nrays, samples=rc.nsamples, step=step, build_seconds=build,
                   render_seconds=float(np.median(times)), resident_bytes_per_sample=4 + 8 * 3 + 4 + 8,
                   mean_alpha=float(rgba[:, 3].mean()))
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
