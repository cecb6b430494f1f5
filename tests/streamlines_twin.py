"""A plain NumPy restatement of the step loop of csrc/stream.hip, operation by operation in IEEE double.

The field is a callable `v(points) -> (values, found)`: `points` is `(M, d)`, `values` `(M, d)` and `found` `(M,)` bool
(False: the point is in no element; its row of `values` is ignored).  The CPU tests pass exact fields, the GPU tests pass
`interpolate()` at the twin's own stage points, so that the twin and the kernel see bitwise equal velocities and every
later operation can be compared bit for bit.  All lines advance together, stage by stage; a line's arithmetic does not
depend on the others.

One step, with `h` the signed step (no fused multiply-add anywhere: NumPy has none):

    k1 = v(x);  k2 = v(x + (0.5*h)*k1);  k3 = v(x + (0.5*h)*k2);  k4 = v(x + h*k3)
    x_new = x + (h/6.0)*(((k1 + 2.0*k2) + 2.0*k3) + k4)

Every stage: no element ends the line at the current x (`OUTSIDE` if the line has no point yet, `LEFT` otherwise); then
`speed = sqrt(v.v)` with the squares added in axis order, and `not speed > min_speed` ends it with `STALLED`; with
`normalize` the stage velocity is `v / speed`.
"""
import numpy as np

MAX_STEPS, LEFT, STALLED, OUTSIDE = range(4)


class TwinLines:
    def __init__(self, points, n, status):
        self.points, self.n, self.status = points, n, status


def trace_twin(v, seeds, h, max_steps, normalize=False, min_speed=0.0):
    seeds = np.asarray(seeds, dtype=np.float64)
    S, d = seeds.shape
    h = float(h)
    points = np.full((S, max_steps + 1, d), np.nan)
    n = np.zeros(S, dtype=np.int32)
    status = np.full(S, MAX_STEPS, dtype=np.int32)
    x = seeds.copy()
    k = np.zeros((S, d))
    acc = np.zeros((S, d))
    active = np.ones(S, dtype=bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for _ in range(max_steps):
            for s in range(4):
                idx = np.flatnonzero(active)
                if idx.size == 0:
                    break
                if s == 0:
                    y = x[idx]
                else:
                    c = h if s == 3 else 0.5 * h
                    y = x[idx] + c * k[idx]
                vals, found = v(y)
                vals, found = np.asarray(vals, dtype=np.float64).reshape(idx.size, d), np.asarray(found, dtype=bool)
                lost = idx[~found]
                status[lost] = np.where(n[lost] == 0, OUTSIDE, LEFT)
                active[lost] = False
                idx, vals = idx[found], vals[found]
                first = idx[n[idx] == 0]                     # the seed has an element: it is the line's first point
                points[first, 0] = x[first]
                n[first] = 1
                sq = vals[:, 0] * vals[:, 0]
                for a in range(1, d):
                    sq = sq + vals[:, a] * vals[:, a]
                speed = np.sqrt(sq)
                ok = speed > min_speed                       # False for NaN
                status[idx[~ok]] = STALLED
                active[idx[~ok]] = False
                idx, vals, speed = idx[ok], vals[ok], speed[ok]
                if normalize:
                    vals = vals / speed[:, None]
                k[idx] = vals
                acc[idx] = vals if s == 0 else acc[idx] + (1.0 if s == 3 else 2.0) * vals
            idx = np.flatnonzero(active)
            x[idx] = x[idx] + (h / 6.0) * acc[idx]
            points[idx, n[idx]] = x[idx]
            n[idx] += 1
    return TwinLines(points, n, status)


def join_twin(back, fwd):
    """`direction="both"`: per seed the backward line reversed and without its duplicate seed, then the forward line."""
    S, m1, d = fwd.points.shape
    points = np.full((S, 2 * m1 - 1, d), np.nan)
    n = np.zeros(S, dtype=np.int32)
    for i in range(S):
        if fwd.n[i] == 0:
            continue
        line = np.concatenate([back.points[i, :back.n[i]][::-1][:-1], fwd.points[i, :fwd.n[i]]])
        points[i, :len(line)] = line
        n[i] = len(line)
    return TwinLines(points, n, np.stack([back.status, fwd.status], axis=1).astype(np.int32))
