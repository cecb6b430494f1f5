"""A NumPy restatement of the triangle caster (multigridbarrier.jl_amd/surface.py, csrc/surface.hip) without its grid:
every ray against every triangle by the documented formulas in the documented operation order, in IEEE double without
fused multiply-adds (NumPy's elementwise products and sums), so that `t`, `u` and `v` agree with the device bit for bit;
the selection of the K nearest hits by `(t, triangle index)`; the shade formula; and the composite of a ray's layers with
its volume samples, written as a merge of two ascending lists.  It never touches the device.
"""
import math
from dataclasses import dataclass

import numpy as np


def normalize_twin(d):
    d = np.asarray(d, dtype=np.float64)
    s = d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return d / np.sqrt(s)[:, None]


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


@dataclass
class Pairs:
    """Every (ray, triangle) pair: `(R, T)` arrays."""
    det: np.ndarray
    u: np.ndarray
    v: np.ndarray
    t: np.ndarray
    ok: np.ndarray          # det finite and non-zero
    hit: np.ndarray


def pairs_twin(points, o, dn, t_min=0.0, t_max=math.inf):
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3, 3)
    o, dn = np.asarray(o, dtype=np.float64), np.asarray(dn, dtype=np.float64)
    v0 = P[None, :, 0, :]
    e1 = (P[:, 1] - P[:, 0])[None]
    e2 = (P[:, 2] - P[:, 0])[None]
    D = dn[:, None, :]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        p = _cross(np.broadcast_to(D, (o.shape[0], P.shape[0], 3)), e2)
        det = _dot(e1, p)
        s = o[:, None, :] - v0
        u = _dot(s, p) / det
        q = _cross(s, e1)
        v = _dot(D, q) / det
        t = _dot(e2, q) / det
        ok = np.isfinite(det) & (det != 0.0)
        hit = ok & (u >= 0.0) & (v >= 0.0) & (u + v <= 1.0) & (t_min <= t) & (t <= t_max)
    return Pairs(det, u, v, t, ok, hit)


def trace_twin(points, o, d, t_min=0.0, t_max=math.inf, K=1):
    """`(t, tri, u, v, pairs)`: the K nearest hits per ray in the order of (t, triangle index); missing entries are
    t = inf, tri = -1, u = v = NaN."""
    dn = normalize_twin(d)
    pr = pairs_twin(points, o, dn, t_min, t_max)
    R = dn.shape[0]
    t = np.full((R, K), np.inf)
    tri = np.full((R, K), -1, dtype=np.int32)
    u, v = np.full((R, K), np.nan), np.full((R, K), np.nan)
    for r in range(R):
        idx = np.nonzero(pr.hit[r])[0]
        order = sorted(idx.tolist(), key=lambda i: (pr.t[r, i], i))[:K]
        for k, i in enumerate(order):
            t[r, k], tri[r, k], u[r, k], v[r, k] = pr.t[r, i], i, pr.u[r, i], pr.v[r, i]
    return t, tri, u, v, pr


def margin_twin(pr, t_min, t_max):
    """The smallest distance from 0 of u, v, 1 - u - v, t - t_min and t_max - t over the pairs with a usable det, and the
    smallest gap in t between two hits of one ray."""
    ok = pr.ok
    m = math.inf
    with np.errstate(invalid="ignore"):
        quantities = (pr.u, pr.v, 1.0 - pr.u - pr.v, pr.t - t_min, t_max - pr.t)
    for q in quantities:
        a = np.abs(q[ok])
        a = a[~np.isnan(a)]
        if a.size:
            m = min(m, float(a.min()))
    gap = math.inf
    for r in range(pr.t.shape[0]):
        th = np.sort(pr.t[r][pr.hit[r]])
        if th.size > 1:
            gap = min(gap, float(np.diff(th).min()))
    return m, gap


def shade_twin(points, dn, tri, u, v, values, table, lo, hi, ambient):
    """(R, K, 4): the layer of every hit, operation by operation as the kernel forms it."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3, 3)
    Tb = np.asarray(table, dtype=np.float64)
    Kt = Tb.shape[0]
    R, K = tri.shape
    out = np.zeros((R, K, 4))
    for r in range(R):
        for k in range(K):
            i = int(tri[r, k])
            if i < 0:
                continue
            uu, vv = float(u[r, k]), float(v[r, k])
            w = (1.0 - uu) - vv
            c = (w * float(values[i, 0]) + uu * float(values[i, 1])) + vv * float(values[i, 2])
            if not math.isfinite(c):
                continue
            sc = min(1.0, max(0.0, (c - lo) / (hi - lo)))
            f = sc * (Kt - 1)
            j = min(int(math.floor(f)), Kt - 2)
            wj = f - j
            row = [float(Tb[j, q]) + wj * (float(Tb[j + 1, q]) - float(Tb[j, q])) for q in range(4)]
            e1, e2 = P[i, 1] - P[i, 0], P[i, 2] - P[i, 0]
            n = _cross(e1, e2)
            nn = n / math.sqrt(float(_dot(n, n)))
            shade = ambient + (1.0 - ambient) * abs(float(_dot(nn, dn[r])))
            alpha = min(1.0, max(0.0, row[3]))
            a_s = alpha * shade
            out[r, k] = [a_s * row[0], a_s * row[1], a_s * row[2], alpha]
    return out


def sample_times(rays, r):
    """The parameters of ray r's samples, formed as the emit kernel forms them."""
    return [float(rays.tmin[r]) + (i + 0.5) * float(rays.h[r]) for i in range(int(rays.n[r]))]


def composite_twin(rays, vals, transfer, lo, hi, t_hit, layer):
    """(R, 4): the samples of `rays` (tests/raycast_twin.py) and the hits of each ray merged by depth: a hit goes before
    sample i iff t_hit <= t_i; the finite hits that remain go after the last sample."""
    Tb = np.asarray(transfer, dtype=np.float64)
    K = Tb.shape[0]
    R = rays.n.size
    out = np.zeros((R, 4))
    for r in range(R):
        h = float(rays.h[r])
        events = [(float(t_hit[r, k]), 0, k) for k in range(t_hit.shape[1]) if math.isfinite(t_hit[r, k])]
        events += [(ti, 1, i) for i, ti in enumerate(sample_times(rays, r))]
        events.sort()                               # a hit at t_hit == t_i sorts before the sample (0 < 1)
        T, C = 1.0, [0.0, 0.0, 0.0]
        for _, kind, i in events:
            if kind == 0:
                for c in range(3):
                    C[c] += T * float(layer[r, i, c])
                T = T * (1.0 - float(layer[r, i, 3]))
                continue
            v = float(vals[int(rays.offsets[r]) + i])
            if not math.isfinite(v):
                continue
            sc = min(1.0, max(0.0, (v - lo) / (hi - lo)))
            f = sc * (K - 1)
            j = min(int(math.floor(f)), K - 2)
            w = f - j
            row = [float(Tb[j, c]) + w * (float(Tb[j + 1, c]) - float(Tb[j, c])) for c in range(4)]
            e = math.exp(-(row[3] * h))
            for c in range(3):
                C[c] += (T * (1.0 - e)) * row[c]
            T = T * e
        out[r] = [C[0], C[1], C[2], 1.0 - T]
    return out


def sample_margin(rays, t_hit):
    """The smallest |t_hit - t_i| over the finite hits and the samples of their rays."""
    m = math.inf
    for r in range(rays.n.size):
        ts = np.array(sample_times(rays, r))
        for th in t_hit[r][np.isfinite(t_hit[r])]:
            if ts.size:
                m = min(m, float(np.abs(ts - th).min()))
    return m
