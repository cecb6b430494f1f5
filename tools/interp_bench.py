"""Time `interpolate` on the device: 4 M random points on fem2d_P2 at L = 9 and 1 M on fem3d (k = 3) at L = 5.

Prints one JSON line per case: wall-clock seconds per call (median of --reps calls after one warm-up; the call includes
the uploads, the location-grid build, the query and the copy back) and the maximum error against the reproduced
polynomial.  With --gradient every call also asks for the gradient at the points (`gradient=True`: the GRAD query
kernels) and the line carries the maximum error of the gradient against the polynomial's.  With --locator every case
also builds one `PointLocator` for the same points and the line carries the seconds of its construction
(`locator_seconds_create`), the median seconds of `evaluate` (`locator_seconds_per_evaluate`, same --reps rule, with the
gradient under --gradient) next to `seconds_per_call` of `interpolate()` in the same process, and whether the two
results are bitwise equal (`bitwise_equal`).  Kernel durations come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/interp_bench.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402


def _bitwise(a, b):
    return a.shape == b.shape and bool(np.array_equal(a, b, equal_nan=True))


def run(name, geom, f, M, reps, rng, df=None, locator=False):
    d = geom.x.shape[2]
    z = f(geom.xflat)
    pts = rng.uniform(-1, 1, (M, d))
    call = (lambda: m.interpolate(geom, z, pts, gradient=True)) if df else (lambda: (m.interpolate(geom, z, pts), None))
    call()                                            # warm-up: context, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        vals, grads = call()
        times.append(time.perf_counter() - t0)
    res = dict(case=name, elements=int(geom.x.shape[1]), points=M, gradient=df is not None,
               seconds_per_call=float(np.median(times)), max_rel_err=float(np.abs(vals - f(pts)).max() / np.abs(z).max()))
    if df:
        exact = df(pts)
        res["max_rel_err_gradient"] = float(np.abs(grads - exact).max() / np.abs(exact).max())
    if locator:
        t0 = time.perf_counter()
        loc = m.PointLocator(geom, pts)
        res["locator_seconds_create"] = time.perf_counter() - t0
        try:
            ev = (lambda: loc.evaluate(z, gradient=True)) if df else (lambda: (loc.evaluate(z), None))
            ev()                                      # warm-up: code objects of the evaluate kernel, result buffers
            times = []
            for _ in range(reps):
                t0 = time.perf_counter()
                lv, lg = ev()
                times.append(time.perf_counter() - t0)
        finally:
            loc.close()
        res["locator_seconds_per_evaluate"] = float(np.median(times))
        res["bitwise_equal"] = _bitwise(lv, vals) and (df is None or _bitwise(lg, grads))
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2", type=int, default=9)
    ap.add_argument("--L3", type=int, default=5)
    ap.add_argument("--gradient", action="store_true", help="also evaluate the gradient at every point")
    ap.add_argument("--locator", action="store_true", help="also time a PointLocator on the same points")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    a = rng.standard_normal(6)
    quad = lambda X: a[0] + a[1] * X[:, 0] + a[2] * X[:, 1] + a[3] * X[:, 0] ** 2 + a[4] * X[:, 0] * X[:, 1] + a[5] * X[:, 1] ** 2
    dquad = lambda X: np.stack([a[1] + 2 * a[3] * X[:, 0] + a[4] * X[:, 1], a[2] + a[4] * X[:, 0] + 2 * a[5] * X[:, 1]], axis=1)
    run(f"fem2d_P2 L={args.L2}", m.subdivide(m.fem2d_P2(), args.L2), quad, 4 * 2 ** 20, args.reps, rng,
        dquad if args.gradient else None, args.locator)
    cub = lambda X: X[:, 0] ** 3 - 2 * X[:, 1] ** 2 * X[:, 2] + X[:, 0] * X[:, 1] * X[:, 2] + 0.5
    dcub = lambda X: np.stack([3 * X[:, 0] ** 2 + X[:, 1] * X[:, 2], -4 * X[:, 1] * X[:, 2] + X[:, 0] * X[:, 2],
                               -2 * X[:, 1] ** 2 + X[:, 0] * X[:, 1]], axis=1)
    run(f"fem3d k=3 L={args.L3}", m.subdivide(m.fem3d(k=3), args.L3), cub, 2 ** 20, args.reps, rng,
        dcub if args.gradient else None, args.locator)


if __name__ == "__main__":
    main()
