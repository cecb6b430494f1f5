"""A NumPy restatement of the segment caster (multigridbarrier.jl_amd/tubes.py, csrc/tubes.hip) without its grid: every
ray against every capsule by the documented formulas in the documented operation order, in IEEE double without fused
multiply-adds (NumPy's elementwise products and sums), so that both sides run the same additions and products and can
differ only in how they round the square roots and the divisions; the selection of the K nearest hits by `(t, segment
index)`; and the shade formula.  It never touches the device.
"""
import math
from dataclasses import dataclass

import numpy as np

from surface_twin import _dot, normalize_twin  # noqa: F401  (normalize_twin is re-exported)

SIDE, CAP_A, CAP_B, NONE = 0, 1, 2, -1
EPS = 2.0 ** -52


@dataclass
class Pairs:
    """Every (ray, segment) pair: `(R, S)` arrays."""
    baba: np.ndarray
    bard: np.ndarray
    baoa: np.ndarray
    A: np.ndarray
    h: np.ndarray            # the side's discriminant
    h2a: np.ndarray          # cap a's
    h2b: np.ndarray          # cap b's
    hs: np.ndarray           # the scales of h, h2a, h2b: the sum of the magnitudes of the two terms each is a difference of
    h2as: np.ndarray
    h2bs: np.ndarray
    y: np.ndarray            # the side's axis coordinate (NaN where A <= 0 or h < 0)
    ts: np.ndarray           # entry parameters of the three pieces, NaN where the piece's root does not exist
    ta: np.ndarray
    tb: np.ndarray
    side_ok: np.ndarray      # the pieces' validity
    a_ok: np.ndarray
    b_ok: np.ndarray
    t: np.ndarray            # the capsule's entry parameter (inf: no valid piece)
    s: np.ndarray
    piece: np.ndarray        # SIDE, CAP_A, CAP_B or NONE
    hit: np.ndarray


def pairs_twin(points, radii, o, dn, t_min=0.0, t_max=math.inf):
    P = np.asarray(points, dtype=np.float64).reshape(-1, 2, 3)
    rad = np.broadcast_to(np.asarray(radii, dtype=np.float64), (P.shape[0],))
    o, dn = np.asarray(o, dtype=np.float64), np.asarray(dn, dtype=np.float64)
    R, S = o.shape[0], P.shape[0]
    a, b = P[None, :, 0, :], P[None, :, 1, :]
    ba = np.broadcast_to(b - a, (R, S, 3))
    oa = o[:, None, :] - a
    ob = o[:, None, :] - b
    D = np.broadcast_to(dn[:, None, :], (R, S, 3))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        baba, bard, baoa, rdoa, oaoa = _dot(ba, ba), _dot(ba, D), _dot(ba, oa), _dot(D, oa), _dot(oa, oa)
        rr = (rad * rad)[None, :]
        A = baba - bard * bard
        B = baba * rdoa - baoa * bard
        Cq = (baba * oaoa - baoa * baoa) - rr * baba
        h = B * B - A * Cq
        hs = B * B + np.abs(A * Cq)
        root = (A > 0.0) & (h >= 0.0)
        ts = np.where(root, (-B - np.sqrt(np.where(root, h, 0.0))) / np.where(root, A, 1.0), np.nan)
        y = baoa + ts * bard
        side_ok = root & (y >= 0.0) & (y <= baba)
        h2a = rdoa * rdoa - (oaoa - rr)
        h2as = rdoa * rdoa + np.abs(oaoa - rr)
        a_ok = h2a >= 0.0
        ta = np.where(a_ok, -rdoa - np.sqrt(np.where(a_ok, h2a, 0.0)), np.nan)
        b2 = _dot(D, ob)
        h2b = b2 * b2 - (_dot(ob, ob) - rr)
        h2bs = b2 * b2 + np.abs(_dot(ob, ob) - rr)
        b_ok = h2b >= 0.0
        tb = np.where(b_ok, -b2 - np.sqrt(np.where(b_ok, h2b, 0.0)), np.nan)
        t = np.full((R, S), np.inf)
        s = np.full((R, S), np.nan)
        piece = np.full((R, S), NONE)
        t, s, piece = np.where(side_ok, ts, t), np.where(side_ok, y / baba, s), np.where(side_ok, SIDE, piece)
        take = a_ok & (ta < t)
        t, s, piece = np.where(take, ta, t), np.where(take, 0.0, s), np.where(take, CAP_A, piece)
        take = b_ok & (tb < t)
        t, s, piece = np.where(take, tb, t), np.where(take, 1.0, s), np.where(take, CAP_B, piece)
        hit = (t < np.inf) & (t_min <= t) & (t <= t_max)
    return Pairs(baba, bard, baoa, A, h, h2a, h2b, hs, h2as, h2bs, y, ts, ta, tb, side_ok, a_ok, b_ok, t, s, piece, hit)


@dataclass
class TwinHits:
    t: np.ndarray            # (R, K)
    segment: np.ndarray      # (R, K) int32
    s: np.ndarray
    piece: np.ndarray        # (R, K): SIDE, CAP_A, CAP_B, NONE
    A: np.ndarray            # per hit, the intermediates of the winning piece (NaN for a missing hit)
    h: np.ndarray            # h on the side, h2 on a cap
    bard: np.ndarray
    baoa: np.ndarray
    baba: np.ndarray
    pairs: Pairs


def trace_twin(points, radii, o, d, t_min=0.0, t_max=math.inf, K=1):
    """The K nearest hits per ray in the order of (t, segment index); missing entries are t = inf, segment = -1,
    s = NaN."""
    dn = normalize_twin(d)
    pr = pairs_twin(points, radii, o, dn, t_min, t_max)
    R = dn.shape[0]
    t = np.full((R, K), np.inf)
    seg = np.full((R, K), -1, dtype=np.int32)
    piece = np.full((R, K), NONE)
    s, A, h, bard, baoa, baba = (np.full((R, K), np.nan) for _ in range(6))
    for r in range(R):
        idx = np.nonzero(pr.hit[r])[0]
        order = sorted(idx.tolist(), key=lambda i: (pr.t[r, i], i))[:K]
        for k, i in enumerate(order):
            t[r, k], seg[r, k], s[r, k], piece[r, k] = pr.t[r, i], i, pr.s[r, i], pr.piece[r, i]
            A[r, k], bard[r, k], baoa[r, k], baba[r, k] = pr.A[r, i], pr.bard[r, i], pr.baoa[r, i], pr.baba[r, i]
            h[r, k] = (pr.h, pr.h2a, pr.h2b)[int(pr.piece[r, i])][r, i]
    return TwinHits(t, seg, s, piece, A, h, bard, baoa, baba, pr)


def piece_of(s, segment):
    """The piece a reported hit lies on, read from s: 0 is cap a, 1 cap b, anything strictly between the side."""
    s = np.asarray(s)
    out = np.full(s.shape, NONE)
    there = np.asarray(segment) >= 0
    out[there & (s == 0.0)] = CAP_A
    out[there & (s == 1.0)] = CAP_B
    out[there & (s > 0.0) & (s < 1.0)] = SIDE
    return out


def t_bound(tw: TwinHits):
    """Per hit, how far the device's t may lie from the twin's: both sides run identical IEEE + - * in the same order, so
    h, B and A agree bitwise and only sqrt and / may round differently, by at most one ulp each.  Through
    t = (-B - sqrt(h)) / A that is eps sqrt(h) / A from the root plus eps |t| from the division, to first order; with a
    factor 2 over the first-order term: 4 eps (|t| + sqrt(h) / A) on the side and 4 eps (|t| + sqrt(h2)) on a cap."""
    with np.errstate(invalid="ignore", divide="ignore"):
        side = 4 * EPS * (np.abs(tw.t) + np.sqrt(tw.h) / tw.A)
        cap = 4 * EPS * (np.abs(tw.t) + np.sqrt(tw.h))
    return np.where(tw.piece == SIDE, side, np.where(tw.piece == NONE, 0.0, cap))


def s_bound(tw: TwinHits):
    """Per hit, the bound on s: exactly 0 on the caps; on the side y = baoa + t bard moves by |bard| bound_t and rounds
    twice, and the division adds eps |s|: (|bard| bound_t + 2 eps (|baoa| + |t bard|)) / baba + eps |s|."""
    bt = t_bound(tw)
    with np.errstate(invalid="ignore", divide="ignore"):
        side = (np.abs(tw.bard) * bt + 2 * EPS * (np.abs(tw.baoa) + np.abs(tw.t * tw.bard))) / tw.baba + EPS * np.abs(tw.s)
    return np.where(tw.piece == SIDE, side, 0.0)


def margin_twin(pr: Pairs, t_min, t_max):
    """`(margin, gap)`: the smallest relative distance of any (ray, segment) pair from a decision -- h, h2 from zero
    (relative to the sum of the magnitudes of the two terms they are differences of), the y of a side whose root exists
    from 0 and baba (relative to baba), a valid piece's entry t from t_min and t_max and two valid pieces' entries from
    each other (relative to max(1, |t|); the two caps of a segment with a == b are one sphere and tie by construction)
    -- and the smallest such distance between the t of two hits of one ray.  No pair is left out."""
    m = math.inf

    def take(q, scale, mask):
        nonlocal m
        with np.errstate(invalid="ignore", divide="ignore"):
            v = (np.abs(q) / scale)[mask]
        v = v[~np.isnan(v)]
        if v.size:
            m = min(m, float(v.min()))

    everything = np.ones(pr.h.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        sphere = pr.baba == 0.0
        take(pr.h, pr.hs, pr.A > 0.0)              # with A <= 0 the side is invalid whatever h is
        take(pr.h2a, pr.h2as, everything)
        take(pr.h2b, pr.h2bs, everything)
        root = ~np.isnan(pr.ts)
        take(pr.y, pr.baba, root)
        take(pr.y - pr.baba, pr.baba, root)
        for tp, ok in ((pr.ts, pr.side_ok), (pr.ta, pr.a_ok), (pr.tb, pr.b_ok)):
            sc = np.maximum(1.0, np.abs(tp))
            take(tp - t_min, sc, ok)
            if math.isfinite(t_max):
                take(tp - t_max, sc, ok)
        for (t1, ok1), (t2, ok2) in (((pr.ts, pr.side_ok), (pr.ta, pr.a_ok)), ((pr.ts, pr.side_ok), (pr.tb, pr.b_ok)),
                                     ((pr.ta, pr.a_ok), (pr.tb, pr.b_ok))):
            take(t1 - t2, np.maximum(1.0, np.abs(t1)), ok1 & ok2 & ~sphere)
    gap = math.inf
    for r in range(pr.t.shape[0]):
        th = np.sort(pr.t[r][pr.hit[r]])
        if th.size > 1:
            gap = min(gap, float((np.diff(th) / np.maximum(1.0, np.abs(th[1:]))).min()))
    return m, gap


def shade_twin(points, o, dn, t, segment, s, values, table, lo, hi, ambient):
    """(R, K, 4): the layer of every hit, operation by operation as the kernel forms it."""
    P = np.asarray(points, dtype=np.float64).reshape(-1, 2, 3)
    Tb = np.asarray(table, dtype=np.float64)
    Kt = Tb.shape[0]
    R, K = segment.shape
    out = np.zeros((R, K, 4))
    for r in range(R):
        for k in range(K):
            i = int(segment[r, k])
            if i < 0:
                continue
            ss, tt = float(s[r, k]), float(t[r, k])
            c = (1.0 - ss) * float(values[i, 0]) + ss * float(values[i, 1])
            if not math.isfinite(c):
                continue
            sc = min(1.0, max(0.0, (c - lo) / (hi - lo)))
            f = sc * (Kt - 1)
            j = min(int(math.floor(f)), Kt - 2)
            wj = f - j
            row = [float(Tb[j, q]) + wj * (float(Tb[j + 1, q]) - float(Tb[j, q])) for q in range(4)]
            x = o[r] + tt * dn[r]
            q = P[i, 0] + ss * (P[i, 1] - P[i, 0])
            n = x - q
            nn = n / math.sqrt(float(_dot(n, n)))
            shade = ambient + (1.0 - ambient) * abs(float(_dot(nn, dn[r])))
            alpha = min(1.0, max(0.0, row[3]))
            a_s = alpha * shade
            out[r, k] = [a_s * row[0], a_s * row[1], a_s * row[2], alpha]
    return out
