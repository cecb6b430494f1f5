"""Time `polylines` on the device: the five level curves of fem2d_P2 at L = 9 (default `refine`, welded with the default
tolerance) and one spiral of 4096 shuffled segments.

Prints one JSON line per case: wall-clock seconds per call (median of --reps calls after one warm-up; the call includes
the upload of the mesh, both sorts, every doubling round and the copy back; the weld before it is not timed), the
segments, lines and points, the doubling rounds and the longest line.  With --host the line also carries the wall-clock of
a plain Python walk of the same mesh (dictionaries and a loop over the edges): a NumPy figure for scale, not a tuned CPU
baseline.  Kernel durations come from a run under `rocprofv3 --kernel-trace --stats -- python tools/polyline_bench.py`.
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
    return np.sin(1.3 * X[:, 0] + 0.4) * np.cos(0.9 * X[:, 1] - 0.2)


def spiral(nseg=4096, seed=11):
    """One polyline spiral as an (S, 2, 2) soup, the segments in a seeded random order and orientation."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, nseg + 1)
    pts = np.stack([(0.2 + 0.8 * t) * np.cos(16 * np.pi * t), (0.2 + 0.8 * t) * np.sin(16 * np.pi * t)], axis=1)
    segs = np.stack([np.arange(nseg), np.arange(nseg) + 1], axis=1)[rng.permutation(nseg)]
    flip = rng.random(nseg) < 0.5
    segs[flip] = segs[flip][:, ::-1]
    return pts[segs]


def python_walk(vertices, cells):
    """The lines of a mesh without junctions by a sequential walk: a list of vertex lists.  (No numbering by lowest segment
    and no arc length: less than `polylines` returns.)"""
    adj = {}
    for s, (a, b) in enumerate(cells.tolist()):
        if a != b:
            adj.setdefault(a, []).append((s, b))
            adj.setdefault(b, []).append((s, a))
    used, lines = set(), []
    starts = [v for v, n in adj.items() if len(n) != 2] + list(adj)
    for v in starts:
        for s, w in adj[v]:
            if s in used:
                continue
            line = [v, w]
            used.add(s)
            while len(adj[w]) == 2 and w != v:
                s, w = adj[w][1] if adj[w][0][0] == s else adj[w][0]
                used.add(s)
                line.append(w)
            lines.append(line)
    return lines


def run(name, mesh, reps, host):
    m.polylines(mesh)                                 # warm-up: context, code objects
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        pl = m.polylines(mesh)
        times.append(time.perf_counter() - t0)
    res = dict(case=name, segments=int(mesh.cells.shape[0]), vertices=int(mesh.vertices.shape[0]), lines=pl.nlines,
               points=int(pl.vertex.shape[0]), closed=int(pl.closed.sum()), dropped=pl.ndropped, rounds=list(pl.rounds),
               longest_line=int(np.diff(pl.offsets).max()) - 1, seconds_per_call=float(np.median(times)))
    if host:
        t0 = time.perf_counter()
        lines = python_walk(mesh.vertices, mesh.cells)
        res["python_walk_seconds"] = time.perf_counter() - t0
        res["python_walk_lines"] = len(lines)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2", type=int, default=9)
    ap.add_argument("--host", action="store_true", help="also time a plain Python walk of the same mesh")
    args = ap.parse_args()
    geom = m.subdivide(m.fem2d_P2(), args.L2)
    run(f"fem2d_P2 L={args.L2}", m.weld(m.isocontour(geom, smooth(geom.xflat), LEVELS)), args.reps, args.host)
    run("spiral 4096", m.weld(spiral(), tol=0.0), args.reps, args.host)


if __name__ == "__main__":
    main()
