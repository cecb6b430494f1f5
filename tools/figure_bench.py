"""Time frames of a trajectory: `FigureRenderer` against a loop of `render_figure` calls, in one process.

The case is that of tools/surface_bench.py (fem3d k = 3 at L = 5, an 800 x 600 pinhole image, the five default
isosurfaces over the trajectory's range) with --frames frames of a smoothly varying field.  `render_figure` is the
unchanged host chain and so the baseline; its loop is timed --loops times to show the run-to-run spread next to the
ratio.  Prints a progress line per stage on stderr and one JSON line on stdout: the soup of the first frame, the
seconds to build the renderer, the median wall-clock seconds per frame of `render`, of `render_rgba8` and of
`render_figure` (per loop), the ratio of the medians, and whether the frames of both paths are bitwise equal.
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
from mgb_amd.surface import REFERENCE_ISOSURFACES  # noqa: E402

EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


def field(X, s):
    """A field that moves smoothly with s in [0, 1]."""
    return (np.sin(1.3 * X[:, 0] + 0.4 + 0.8 * s) * np.cos(0.9 * X[:, 1] - 0.2 - 0.5 * s)
            + 0.35 * np.sin(1.1 * X[:, 2] + 0.3 + 1.1 * s))


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--loops", type=int, default=2)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--L", type=int, default=5)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=600)
    args = ap.parse_args()
    geom = m.subdivide(m.fem3d(k=args.k), args.L)
    X = geom.xflat
    U = np.stack([field(X, j / max(1, args.frames - 1)) for j in range(args.frames)], axis=1)
    lo, hi = float(U.min()), float(U.max())
    levels = np.array(REFERENCE_ISOSURFACES) * (hi - lo) + lo
    size = (args.width, args.height)
    cols = [np.ascontiguousarray(U[:, j]) for j in range(args.frames)]
    note("mesh", X.shape, "frames", args.frames)

    t0 = time.perf_counter()
    fr = m.FigureRenderer(geom, EYE, TARGET, size=size, isosurfaces=levels, clim=(lo, hi))
    build = time.perf_counter() - t0
    note("renderer built", build)
    with fr:
        fr.render(cols[0])                                        # warm-up: code objects, buffers
        triangles, pairs = fr.ntriangles, fr.npairs
        res_t, res = [], []
        for u in cols:
            t0 = time.perf_counter()
            res.append(fr.render(u))
            res_t.append(time.perf_counter() - t0)
        note("render", res_t)
        byte_t = []
        for u in cols:
            t0 = time.perf_counter()
            q = fr.render_rgba8(u)
            byte_t.append(time.perf_counter() - t0)
        note("render_rgba8", byte_t)

    m.render_figure(geom, cols[0], EYE, TARGET, size=(64, 48), isosurfaces=levels, clim=(lo, hi))    # warm-up
    loops, same = [], True
    for _ in range(args.loops):
        times = []
        for j, u in enumerate(cols):
            t0 = time.perf_counter()
            img = m.render_figure(geom, u, EYE, TARGET, size=size, isosurfaces=levels, clim=(lo, hi))
            times.append(time.perf_counter() - t0)
            same = same and np.array_equal(img, res[j])
        note("render_figure", times)
        loops.append(float(np.median(times)))
    resident, baseline = float(np.median(res_t)), float(np.median(loops))
    out = dict(case=f"fem3d k={args.k} L={args.L} {args.width}x{args.height}, {len(levels)} isosurfaces, {args.frames} frames",
               triangles=triangles, pairs=pairs, build_seconds=build, render_seconds=resident,
               render_rgba8_seconds=float(np.median(byte_t)), render_figure_seconds=baseline,
               render_figure_seconds_per_loop=loops, ratio=baseline / resident, bitwise_equal=bool(same),
               mean_alpha=float(res[-1][..., 3].mean()), mean_byte=float(q.mean()))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
