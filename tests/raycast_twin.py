"""A NumPy / plain-Python restatement of the ray caster (multigridbarrier.jl_amd/raycast.py, csrc/raycast.hip): the
directions, the clip box, the slab test, the samples, and the integration and compositing loops, operation by operation
in IEEE double without fused multiply-adds (Python floats), so that the samples, the offsets and the steps agree with
the device bit for bit.  It never touches the device: the sample values come from the caller, either an exact field
(tests/test_raycast.py) or `interpolate()` at the twin's own samples (tests/test_gpu_raycast.py).
"""
import math
from dataclasses import dataclass

import numpy as np

QK_BOX_PAD = 0.125
MAX_COUNT = 2.0 ** 31


def clip_box_twin(geom):
    """(2, d): per-axis min and max of the nodes, widened by 1/8 of the extent per side for Q_k with k >= 2."""
    x = geom.xflat
    lo, hi = x.min(axis=0), x.max(axis=0)
    k = getattr(geom.discretization, "k", None)
    if type(geom.discretization).__name__ == "TensorFEM" and k >= 2:
        ext = hi - lo
        lo, hi = lo - QK_BOX_PAD * ext, hi + QK_BOX_PAD * ext
    return np.stack([lo, hi])


def diagonal_twin(box):
    ext = box[1] - box[0]
    return math.sqrt(float(np.sum(ext * ext)))


def default_transfer_twin(box, K=256):
    ramp = np.arange(K) / (K - 1)
    return np.stack([ramp, ramp, ramp, ramp * (4.0 / diagonal_twin(box))], axis=1)


@dataclass
class Rays:
    dn: np.ndarray        # (R, d) normalised directions
    tmin: np.ndarray      # (R,) first parameter (0.0 for a miss)
    chord: np.ndarray     # (R,) tmax - tmin (0.0 for a miss)
    ratio: np.ndarray     # (R,) (tmax - tmin) / step (NaN for a miss)
    n: np.ndarray         # (R,) int64 samples per ray
    h: np.ndarray         # (R,) step per ray (0.0 for a miss)
    offsets: np.ndarray   # (R + 1,) int64
    pts: np.ndarray       # (S, d)

    def half_integer_margin(self):
        """The smallest distance of (tmax - tmin)/step from a half-integer over the rays that hit (inf if none does)."""
        r = self.ratio[self.n > 0]
        return float(np.abs(r - np.floor(r) - 0.5).min()) if r.size else math.inf


def rays_twin(box, o, d, step, t_min=0.0, t_max=math.inf):
    o, d = np.asarray(o, dtype=np.float64), np.asarray(d, dtype=np.float64)
    R, D = o.shape
    step, t_min, t_max = float(step), float(t_min), float(t_max)
    dn = np.empty((R, D))
    tmin_a, chord, ratio, h_a = np.zeros(R), np.zeros(R), np.full(R, np.nan), np.zeros(R)
    n_a = np.zeros(R, dtype=np.int64)
    rows = []
    for r in range(R):
        s = float(d[r, 0]) * float(d[r, 0])
        for a in range(1, D):
            s = s + float(d[r, a]) * float(d[r, a])
        nrm = math.sqrt(s)
        dr = [float(d[r, a]) / nrm for a in range(D)]
        dn[r] = dr
        tmin, tmax, miss = t_min, t_max, False
        for a in range(D):
            oa = float(o[r, a])
            if dr[a] != 0.0:
                t1 = (float(box[0, a]) - oa) / dr[a]
                t2 = (float(box[1, a]) - oa) / dr[a]
                tmin = max(tmin, min(t1, t2))
                tmax = min(tmax, max(t1, t2))
            elif not (float(box[0, a]) <= oa <= float(box[1, a])):
                miss = True
        if miss or not tmax > tmin:
            continue
        length = tmax - tmin
        c = math.floor(length / step + 0.5)
        n = int(MAX_COUNT) if c >= MAX_COUNT else (int(c) if c >= 1 else 1)
        h = length / float(n)
        tmin_a[r], chord[r], ratio[r], h_a[r], n_a[r] = tmin, length, length / step, h, n
        for i in range(n):
            t = tmin + (i + 0.5) * h
            rows.append([float(o[r, a]) + t * dr[a] for a in range(D)])
    offsets = np.concatenate([[0], np.cumsum(n_a)]).astype(np.int64)
    pts = np.array(rows, dtype=np.float64).reshape(-1, D)
    return Rays(dn, tmin_a, chord, ratio, n_a, h_a, offsets, pts)


def integrate_twin(rays, vals):
    """(R,) or (R, ncomp): h * (the finite values added in sample order)."""
    V = np.asarray(vals, dtype=np.float64)
    single = V.ndim == 1
    V = V.reshape(V.shape[0], -1)
    R = rays.n.size
    out = np.zeros((R, V.shape[1]))
    for r in range(R):
        for c in range(V.shape[1]):
            acc = 0.0
            for s in range(rays.offsets[r], rays.offsets[r + 1]):
                v = float(V[s, c])
                if math.isfinite(v):
                    acc += v
            out[r, c] = float(rays.h[r]) * acc
    return out[:, 0] if single else out


def render_twin(rays, vals, transfer, lo, hi):
    """(R, 4): front-to-back emission-absorption compositing in the operation order of the kernel."""
    Tb = np.asarray(transfer, dtype=np.float64)
    K = Tb.shape[0]
    lo, hi = float(lo), float(hi)
    R = rays.n.size
    out = np.zeros((R, 4))
    for r in range(R):
        h = float(rays.h[r])
        T, C = 1.0, [0.0, 0.0, 0.0]
        for s in range(rays.offsets[r], rays.offsets[r + 1]):
            v = float(vals[s])
            if not math.isfinite(v):
                continue
            sc = min(1.0, max(0.0, (v - lo) / (hi - lo)))
            f = sc * (K - 1)
            j = min(int(math.floor(f)), K - 2)
            w = f - j
            row = [float(Tb[j, c]) + w * (float(Tb[j + 1, c]) - float(Tb[j, c])) for c in range(4)]
            e = math.exp(-(row[3] * h))
            alpha = 1.0 - e
            for c in range(3):
                C[c] += (T * alpha) * row[c]
            T = T * e
        out[r] = [C[0], C[1], C[2], 1.0 - T]
    return out
