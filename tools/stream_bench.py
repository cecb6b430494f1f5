"""Time `StreamTracer.trace` on the device: 10^5 seeds of 256 steps on fem2d_P2 at L = 9 and on fem3d (k = 3) at L = 5.

Prints one JSON line per case: wall-clock seconds per `trace` call (median of --reps calls after one warm-up; the call
includes the upload of the seeds and the copy back of the lines, not the construction of the tracer, which is reported
once as `seconds_create`), how the lines ended, the lane-steps taken (the steps the lines actually made:
`sum(max(n - 1, 0))`) and the points of one fused value-only `interpolate()` call on the same mesh, so that a run under

    rocprofv3 --kernel-trace --stats -- python tools/stream_bench.py

holds, in one session, the duration of the `trace_lines` kernel next to that of the fused `query_*` kernel.  A step is four
queries, so the expected ratio of kernel time per lane-step to kernel time per query point is about 4; `tools/stream_bench.py
--stats FILE` reads the profiler's kernel statistics (CSV) together with the JSON lines of the same run (--json FILE) and
prints that ratio.  The field turns about the origin, so most lines stay in the mesh for all 256 steps.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402


def field(X):
    x, y = X[:, 0], X[:, 1]
    cols = [-y + 0.25 * np.sin(2.0 * x), x + 0.25 * np.sin(2.0 * y)]
    if X.shape[1] == 3:
        cols.append(-0.5 * X[:, 2] + 0.2 * np.sin(x * y))
    return np.stack(cols, axis=1)


def run(name, geom, S, steps, step, reps, rng):
    d = geom.x.shape[2]
    z = field(geom.xflat)
    seeds = rng.uniform(-0.9, 0.9, (S, d))
    t0 = time.perf_counter()
    st = m.StreamTracer(geom, z)
    create = time.perf_counter() - t0
    try:
        st.trace(seeds, step=step, max_steps=steps)          # warm-up: code objects, result buffers
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            s = st.trace(seeds, step=step, max_steps=steps)
            times.append(time.perf_counter() - t0)
    finally:
        st.close()
    pts = rng.uniform(-1, 1, (S * 4, d))
    m.interpolate(geom, z, pts)                              # the fused value-only query kernel, d components
    print(json.dumps(dict(case=name, elements=int(geom.x.shape[1]), seeds=S, max_steps=steps, step=step,
                          seconds_create=create, seconds_per_trace=float(np.median(times)),
                          lane_steps=int(np.maximum(s.n.astype(np.int64) - 1, 0).sum()),
                          status_counts=[int(c) for c in np.bincount(s.status, minlength=4)],
                          traces=reps + 1, query_points=int(pts.shape[0]), query_calls=1)), flush=True)


def ratio(stats_csv, json_path):
    """Kernel time per lane-step over kernel time per query point, per case, from the profiler's kernel statistics."""
    rows = list(csv.DictReader(open(stats_csv)))
    cases = [json.loads(ln) for ln in open(json_path) if ln.startswith("{")]

    def total_ns(*fragments):
        return sum(float(r["TotalDurationNs"]) for r in rows if all(f in r["Name"] for f in fragments))
    for c, (trace_k, query_k) in zip(cases, ((("trace_lines", "SimplexField"), ("query_simplex",)),
                                             (("trace_lines", "QkField"), ("query_qk",)))):
        per_step = total_ns(*trace_k) / (c["traces"] * c["lane_steps"])
        per_point = total_ns(*query_k) / (c["query_calls"] * c["query_points"])
        print(f"{c['case']}: trace_lines {per_step:.3f} ns per lane-step, fused value-only query {per_point:.3f} ns per "
              f"point, ratio {per_step / per_point:.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2", type=int, default=9)
    ap.add_argument("--L3", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--stats", help="kernel statistics CSV of a profiled run: print the ratio instead of running")
    ap.add_argument("--json", help="the JSON lines the profiled run printed")
    args = ap.parse_args()
    if args.stats:
        return ratio(args.stats, args.json)
    rng = np.random.default_rng(0)
    run(f"fem2d_P2 L={args.L2}", m.subdivide(m.fem2d_P2(), args.L2), args.seeds, args.steps, 0.01, args.reps, rng)
    run(f"fem3d k=3 L={args.L3}", m.subdivide(m.fem3d(k=3), args.L3), args.seeds, args.steps, 0.01, args.reps, rng)


if __name__ == "__main__":
    main()
