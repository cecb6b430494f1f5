"""Time `Quadrature.integrate` on the device: fem2d_P2 L = 9 (131,072 elements) with 1 and 16 columns, and fem3d k = 3
L = 5 (4,096 elements) with n = 4 points per axis (the basis tables staged in LDS) and the default n = 5 (read through L2).

Prints one JSON line per case: the device milliseconds of the element kernel and of the reduction over the elements
(HIP events on the object's stream, `Quadrature.last_times()`; the median over --reps warm calls), the wall-clock
seconds of a whole call (uploads of z, both launches, the copy back), the bytes one pass reads and the rate that makes,
and, for information, the wall-clock seconds of the host's `geom.w @ F(geom.operators)` for the same integrals.  There
is no pass / fail threshold.  Kernel durations per instantiation come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/integrate_bench.py`.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402


def host_reference(geom, Z, kind, p, s):
    """geom.w @ F / s column by column, as a user without integrate() would write it; seconds and the values."""
    t0 = time.perf_counter()
    ops = geom.operators
    out = []
    for j in range(Z.shape[1]):
        z = Z[:, j]
        if kind == "lp":
            F = np.abs(z) ** p
        else:
            g2 = sum(ops[a].matvec(z) ** 2 for a in ("dx", "dy", "dz")[:geom.x.shape[2]])
            F = g2 ** (0.5 * p)
        out.append(geom.w @ F / s)
    return time.perf_counter() - t0, np.array(out)


def run(name, geom, ncol, kind, p, reps, s, order=None):
    rng = np.random.default_rng(0)
    X = geom.xflat
    Z = np.stack([np.sin(2.0 * X.sum(axis=1) + j) + 0.01 * rng.standard_normal(X.shape[0]) for j in range(ncol)], axis=1)
    with m.Quadrature(geom, order=order) as q:
        pl = q.plan()
        q.integrate(Z, kind=kind, p=p)                        # warm-up: code object, buffers
        el, red, wall = [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            val = q.integrate(Z, kind=kind, p=p)
            wall.append(time.perf_counter() - t0)
            t = q.last_times()
            el.append(t["element_ms"])
            red.append(t["reduce_ms"])
        again = q.integrate(Z, kind=kind, p=p)
        N, Q, P = q.n_elements, q.n_points, q.phi.shape[1]
    with m.Quadrature(geom, rule="nodal") as qn:
        nodal = qn.integrate(Z, kind=kind, p=p)
    host_s, host_val = host_reference(geom, Z, kind, p, s)
    read = 8 * (X.size + Z.size)                              # one pass: the nodes and z, each once
    el_ms = float(np.median(el))
    print(json.dumps({
        "case": name, "kind": kind, "p": p, "elements": N, "nodes": P, "points": Q, "ncol": ncol,
        "G": pl["G"], "tables_lds": pl["tables_lds"], "lds_bytes": pl["lds"], "grid": pl["grid"],
        "element_kernel_ms": el_ms, "reduce_ms": float(np.median(red)), "call_wall_s": float(np.median(wall)),
        "bytes_read": read, "read_GBps": read / (el_ms * 1e-3) / 1e9,
        "bitwise_repeat": bool(np.array_equal(np.asarray(val).view(np.uint64), np.asarray(again).view(np.uint64))),
        "host_w_dot_F_s": host_s, "nodal_vs_host_rel": float(np.max(np.abs(nodal - host_val) / np.abs(host_val))),
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--L2d", type=int, default=9, help="subdivision level of the fem2d_P2 case")
    ap.add_argument("--L3d", type=int, default=5, help="subdivision level of the fem3d k = 3 case")
    a = ap.parse_args()
    g2 = m.subdivide(m.fem2d_P2(), a.L2d)
    run(f"fem2d_P2_L{a.L2d}", g2, 1, "w1p", 1.5, a.reps, 2.0)
    run(f"fem2d_P2_L{a.L2d}", g2, 16, "w1p", 1.5, a.reps, 2.0)
    run(f"fem2d_P2_L{a.L2d}", g2, 1, "lp", 2.0, a.reps, 2.0)
    g3 = m.subdivide(m.fem3d(k=3), a.L3d)
    run(f"fem3d_k3_L{a.L3d}_n4", g3, 1, "w1p", 1.5, a.reps, 1.0, order=4)
    run(f"fem3d_k3_L{a.L3d}_n5", g3, 1, "w1p", 1.5, a.reps, 1.0)


if __name__ == "__main__":
    main()
