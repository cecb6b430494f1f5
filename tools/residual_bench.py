"""Time `ResidualEstimator` on the device: fem2d_P2 L = 9 (131,072 elements) and fem3d k = 2 L = 5 (4,096 elements), each
at the default order, next to `Quadrature.integrate(kind="w1p")` of the same shape, order and exponent in the same
process: the two kernels read the same nodes and z, with 1 + d table rows per node against 1 + d + d (d + 1) / 2.

Prints one JSON line per case: the device milliseconds of the element-residual kernel and of the reduction over the
elements for `interior`, of the pointwise kernel for `strong_residual` (HIP events on the object's stream,
`ResidualEstimator.last_times()`; the median over --reps warm calls), the same two figures of the quadrature, the
wall-clock seconds of whole `interior` and `estimate` calls, and the plans.  With --effectivity L0 it then solves
-lap u = f, u = cos(pi x / 2) cos(pi y / 2) on fem2d_P2 at the levels L0, L0 + 1, L0 + 2 with `mgb_solve` (p = 2) and
prints sqrt(total) / |u - u_h|_{1,2}, the denominator from `norm(kind="w1p", minus=grad u)`.  There is no pass / fail
threshold.  Kernel durations per instantiation come from a run under
`rocprofv3 --kernel-trace --stats -- python tools/residual_bench.py`.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402


def run(name, geom, p, reps):
    X = geom.xflat
    z = np.sin(2.0 * X.sum(axis=1)) + 0.3 * X[:, 0] ** 2
    f = np.cos(X[:, 0]) + 0.3 * X[:, 1]
    with m.ResidualEstimator(geom) as est:
        pl = est.plan()
        est.interior(z, f, p=p)                               # warm-up: code object, buffers
        est.strong_residual(z, f, p=p)
        est.estimate(z, f, p=p)
        el, red, pw, wall, wall_est = [], [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            val = est.interior(z, f, p=p)
            wall.append(time.perf_counter() - t0)
            t = est.last_times()
            el.append(t["element_ms"])
            red.append(t["reduce_ms"])
            est.strong_residual(z, f, p=p)
            pw.append(est.last_times()["element_ms"])
            t0 = time.perf_counter()
            est.estimate(z, f, p=p)
            wall_est.append(time.perf_counter() - t0)
        again = est.interior(z, f, p=p)
        N, Q, P, order = est.n_elements, est.n_points, est.phi.shape[1], est.order
    with m.Quadrature(geom, order=order) as q:
        qp = q.plan()
        q.integrate(z, kind="w1p", p=p)
        qel, qred = [], []
        for _ in range(reps):
            q.integrate(z, kind="w1p", p=p)
            t = q.last_times()
            qel.append(t["element_ms"])
            qred.append(t["reduce_ms"])
    print(json.dumps({
        "case": name, "p": p, "elements": N, "nodes": P, "points": Q, "order": order,
        "G": pl["G"], "tables_lds": pl["tables_lds"], "lds_bytes": pl["lds"], "table_bytes": pl["table_bytes"], "grid": pl["grid"],
        "residual_kernel_ms": float(np.median(el)), "reduce_ms": float(np.median(red)),
        "pointwise_kernel_ms": float(np.median(pw)), "interior_wall_s": float(np.median(wall)),
        "estimate_wall_s": float(np.median(wall_est)),
        "quad_w1p_kernel_ms": float(np.median(qel)), "quad_reduce_ms": float(np.median(qred)),
        "quad_tables_lds": qp["tables_lds"], "quad_lds_bytes": qp["lds"], "quad_table_bytes": qp["table_bytes"],
        "bitwise_repeat": bool(np.array_equal(val[0], again[0]) and val[1] == again[1]),
    }))


def effectivity(L):
    """One p = 2 solve of -lap u = f with u = cos(pi x / 2) cos(pi y / 2) on fem2d_P2 at level L.  The solver minimises
    int s + f_u u with s >= |grad u|^2, that is -2 lap u + f_u = 0: f_u = -pi^2 u, and the estimator's source is
    f = -f_u / 2 = (pi^2 / 2) u."""
    h = 0.5 * math.pi
    exact = lambda X: np.cos(h * X[..., 0]) * np.cos(h * X[..., 1])
    geom = m.subdivide(m.fem2d_P2(), L)
    prob = m.assemble(m.amg(geom), p=2.0,
                      f=lambda x: np.array([-math.pi ** 2 * math.cos(h * x[0]) * math.cos(h * x[1]), 0.0, 0.0, 1.0]),
                      g=lambda x: np.array([math.cos(h * x[0]) * math.cos(h * x[1]), 100.0]))
    sol = m.mgb_solve(prob)
    z = np.ascontiguousarray(sol.z[:, 0])
    with m.ResidualEstimator(geom) as est:
        pts = est.points()
        src = 0.5 * math.pi ** 2 * exact(pts)
        eta2, total = est.estimate(z, src, p=2.0)
        inner, itot = est.interior(z, src, p=2.0)
    with m.Quadrature(geom) as q:
        qp = q.points()
        G = np.stack([-h * np.sin(h * qp[..., 0]) * np.cos(h * qp[..., 1]), -h * np.cos(h * qp[..., 0]) * np.sin(h * qp[..., 1])], axis=2)
        err = q.norm(z, p=2.0, kind="w1p", minus=G)
    print(json.dumps({"case": f"effectivity_fem2d_P2_L{L}", "elements": int(geom.x.shape[1]), "eta": math.sqrt(total),
                      "interior_part": math.sqrt(itot), "h1_seminorm_error": float(err), "effectivity": math.sqrt(total) / float(err)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--L2d", type=int, default=9, help="subdivision level of the fem2d_P2 case")
    ap.add_argument("--L3d", type=int, default=5, help="subdivision level of the fem3d k = 2 case")
    ap.add_argument("--effectivity", type=int, default=0, help="first of three consecutive levels of the p = 2 solves (0: none)")
    a = ap.parse_args()
    run(f"fem2d_P2_L{a.L2d}", m.subdivide(m.fem2d_P2(), a.L2d), 2.0, a.reps)
    run(f"fem2d_P2_L{a.L2d}", m.subdivide(m.fem2d_P2(), a.L2d), 1.5, a.reps)
    run(f"fem3d_k2_L{a.L3d}", m.subdivide(m.fem3d(k=2), a.L3d), 2.0, a.reps)
    run(f"fem3d_k2_L{a.L3d}", m.subdivide(m.fem3d(k=2), a.L3d), 1.5, a.reps)
    for L in range(a.effectivity, a.effectivity + 3 if a.effectivity else 0):
        effectivity(L)


if __name__ == "__main__":
    main()
