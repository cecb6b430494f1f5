"""Time `isocontour` on the device: 5 levels on fem2d_P2 at L = 9 and on fem3d (k = 3) at L = 5, default `refine`.

Prints one JSON line per case: wall-clock seconds per call (median of --reps calls after one warm-up; the call includes
the uploads, both passes, the scan and the copy back), the number of simplices and the measure per level.  With --twin
the line also carries the wall-clock of the NumPy twin of the tests (tests/contour_twin.py) on the same input: a NumPy
figure for orientation, not a tuned CPU baseline.  Kernel durations come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/contour_bench.py`.
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


def run(name, geom, reps, twin):
    z = smooth(geom.xflat)
    m.isocontour(geom, z, LEVELS)                     # warm-up: context, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        c = m.isocontour(geom, z, LEVELS)
        times.append(time.perf_counter() - t0)
    res = dict(case=name, elements=int(geom.x.shape[1]), levels=int(LEVELS.size), simplices=int(c.level.size),
               seconds_per_call=float(np.median(times)), measure=[float(v) for v in c.measure()])
    if twin:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from contour_twin import isocontour_twin
        t0 = time.perf_counter()
        t = isocontour_twin(geom, z, LEVELS)
        res["numpy_twin_seconds"] = time.perf_counter() - t0
        res["same_simplices_as_twin"] = bool(np.array_equal(t.level, c.level) and np.array_equal(t.element, c.element))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2", type=int, default=9)
    ap.add_argument("--L3", type=int, default=5)
    ap.add_argument("--twin", action="store_true", help="also time the NumPy twin on the same input")
    args = ap.parse_args()
    run(f"fem2d_P2 L={args.L2}", m.subdivide(m.fem2d_P2(), args.L2), args.reps, args.twin)
    run(f"fem3d k=3 L={args.L3}", m.subdivide(m.fem3d(k=3), args.L3), args.reps, args.twin)


if __name__ == "__main__":
    main()
