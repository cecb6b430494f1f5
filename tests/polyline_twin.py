"""A sequential Python restatement of `polylines()` by a different algorithm, which the device is compared against.

The device ranks directed half-edges by pointer doubling (csrc/polyline.hip).  Here the lines are walked one edge at a
time: duplicates and degenerate segments are dropped with a dictionary, every open line is walked from a node until the
next node, the edges that remain form cycles and are walked from their lowest vertex, and arc lengths are `np.cumsum`
running sums.  The semantics are fixed so that the two give the same integers:

- segment `s` is dropped if its two vertices are equal, or if a lower-numbered segment that is not dropped joins the same
  two vertices; the others are edges;
- a vertex with two edges is interior, any other vertex with an edge is a node; edges that share an interior vertex
  belong to one line;
- lines are numbered by their lowest segment; an open line starts at the end with the smaller vertex number, with equal
  ends along the end edge with the lower segment number; a closed line starts at its lowest vertex and goes on to the
  smaller of that vertex's two neighbours;
- the length of an edge is `sqrt((dx*dx + dy*dy) [+ dz*dz])`, products and sums rounded separately.
"""
from dataclasses import dataclass

import numpy as np


@dataclass
class TwinLines:
    offsets: np.ndarray
    vertex: np.ndarray
    segment: np.ndarray
    closed: np.ndarray
    arclength: np.ndarray
    length: np.ndarray
    ndropped: int


def edge_lengths(X):
    """(n,) lengths between the consecutive rows of X (n + 1, e)."""
    d = X[1:] - X[:-1]
    q = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    if X.shape[1] == 3:
        q = q + d[:, 2] * d[:, 2]
    return np.sqrt(q)


def polylines_twin(vertices, cells) -> TwinLines:
    X = np.asarray(vertices, dtype=np.float64)
    cells = np.asarray(cells).reshape(-1, 2)
    V, S = X.shape[0], cells.shape[0]

    seen, edges = set(), []
    for s in range(S):
        a, b = int(cells[s, 0]), int(cells[s, 1])
        key = (min(a, b), max(a, b))
        if a == b or key in seen:
            continue
        seen.add(key)
        edges.append(s)
    adj = [[] for _ in range(V)]                 # (segment, other vertex), ascending segment
    for s in edges:
        a, b = int(cells[s, 0]), int(cells[s, 1])
        adj[a].append((s, b))
        adj[b].append((s, a))

    used = set()

    def walk(v, s, w):
        """From v along segment s to w and on through interior vertices, until a node or v comes back."""
        verts, segs = [v, w], [s]
        used.add(s)
        while len(adj[w]) == 2 and w != v:
            s, w = [t for t in adj[w] if t[0] != segs[-1]][0]
            used.add(s)
            segs.append(s)
            verts.append(w)
        return verts, segs

    lines = []                                   # (lowest segment, vertices, segments, closed)
    for v in range(V):
        if len(adj[v]) in (0, 2):
            continue
        for s, w in adj[v]:
            if s in used:
                continue
            verts, segs = walk(v, s, w)
            if verts[-1] < verts[0] or (verts[-1] == verts[0] and segs[-1] < segs[0]):
                verts, segs = verts[::-1], segs[::-1]
            lines.append((min(segs), verts, segs, 0))
    for s in edges:                              # what is left is cycles
        if s in used:
            continue
        cyc, _ = walk(int(cells[s, 0]), s, int(cells[s, 1]))
        v0 = min(cyc)
        s1, w1 = min(adj[v0], key=lambda t: t[1])
        verts, segs = walk(v0, s1, w1)
        assert verts[-1] == v0 and len(segs) >= 3
        lines.append((min(segs), verts, segs, 1))
    lines.sort(key=lambda t: t[0])

    offsets = np.zeros(len(lines) + 1, dtype=np.int64)
    vertex, segment, arc = [], [], []
    for l, (_, verts, segs, _) in enumerate(lines):
        offsets[l + 1] = offsets[l] + len(verts)
        vertex += verts
        segment += segs + [-1]
        arc.append(np.concatenate([[0.0], np.cumsum(edge_lengths(X[verts]))]))
    arclength = np.concatenate(arc) if arc else np.zeros(0)
    return TwinLines(offsets, np.array(vertex, dtype=np.int32), np.array(segment, dtype=np.int32),
                     np.array([c for *_, c in lines], dtype=np.uint8), arclength,
                     arclength[offsets[1:] - 1] if lines else np.zeros(0), S - len(edges))


def sample_twin(points, data, offsets, arclength, line, s):
    """`Polylines.at()` restated: `(points (Q, e), data (Q, C) or None)` for the queries `(line, s)`."""
    X = np.asarray(points, dtype=np.float64)
    D = None if data is None else np.asarray(data, dtype=np.float64)
    line, s = np.broadcast_arrays(np.asarray(line), np.asarray(s, dtype=np.float64))
    out = np.empty((line.size, X.shape[1]))
    od = None if D is None else np.empty((line.size, D.shape[1]))
    for q, (l, sq) in enumerate(zip(line.reshape(-1), s.reshape(-1))):
        o0, o1 = int(offsets[l]), int(offsets[l + 1])
        a = arclength[o0:o1]
        n = o1 - o0 - 1
        sq = min(max(sq, 0.0), a[n])
        j = int(np.searchsorted(a[:n], sq, side="right")) - 1
        d = a[j + 1] - a[j]
        t = 0.0 if d == 0.0 else (sq - a[j]) / d
        out[q] = X[o0 + j] + t * (X[o0 + j + 1] - X[o0 + j])
        if D is not None:
            od[q] = D[o0 + j] + t * (D[o0 + j + 1] - D[o0 + j])
    return out, od
