"""Time `Faces` on the device: fem2d_P2 L = 9 (131,072 elements) and fem3d k = 3 L = 5 (4,096 elements).

Prints one JSON line per case: the device milliseconds of the topology build, of the face kernel and of the reduction
for `integrate` (boundary flux) and of the face kernel for `jumps` (HIP events on the object's stream,
`Faces.last_times()`; the median over --reps warm calls), the wall-clock seconds of the whole calls and of the
construction, and, for information, the wall-clock seconds of the host's `find_boundary` on the same mesh, whose node
pairs are compared with `boundary_nodes()`.  There is no pass / fail threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402


def run(name, geom, p, reps):
    X = geom.xflat
    rng = np.random.default_rng(0)
    z = np.sin(2.0 * X.sum(axis=1)) + 0.01 * rng.standard_normal(X.shape[0])
    t0 = time.perf_counter()
    fc = m.Faces(geom)
    build_s = time.perf_counter() - t0
    with fc:
        topo_ms = fc.last_times()["topology_ms"]
        fc.integrate(z, p=p)
        fc.jumps(z, p=p)                                    # warm-up: code objects, buffers
        ik, ir, iw, jk, jw = [], [], [], [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            v = fc.integrate(z, kind="flux", p=p)
            iw.append(time.perf_counter() - t0)
            t = fc.last_times()
            ik.append(t["face_ms"])
            ir.append(t["reduce_ms"])
            t0 = time.perf_counter()
            J = fc.jumps(z, kind="flux", p=p)
            jw.append(time.perf_counter() - t0)
            jk.append(fc.last_times()["face_ms"])
        again = fc.integrate(z, kind="flux", p=p)
        pb, pi = fc.plan(1), fc.plan(2)
        t0 = time.perf_counter()
        nodes = fc.boundary_nodes()
        nodes_s = time.perf_counter() - t0
        B, I, Qf = fc.n_boundary, fc.n_interior, fc.n_points
    t0 = time.perf_counter()
    host = m.find_boundary(geom)
    host_s = time.perf_counter() - t0
    print(json.dumps({
        "case": name, "p": p, "elements": int(geom.x.shape[1]), "nodes": int(geom.x.shape[0]), "points_per_face": Qf,
        "boundary_faces": B, "interior_faces": I, "topology_ms": topo_ms, "construct_wall_s": build_s,
        "integrate_face_ms": float(np.median(ik)), "integrate_reduce_ms": float(np.median(ir)),
        "integrate_wall_s": float(np.median(iw)), "jumps_face_ms": float(np.median(jk)), "jumps_wall_s": float(np.median(jw)),
        "boundary_plan": pb, "interior_plan": pi, "bitwise_repeat": bool(np.float64(v).view(np.uint64) == np.float64(again).view(np.uint64)),
        "jump_sum": float(J.sum()), "host_find_boundary_s": host_s, "boundary_nodes_s": nodes_s,
        "boundary_nodes_equal_find_boundary": nodes == host,
    }))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--L2d", type=int, default=9, help="subdivision level of the fem2d_P2 case")
    ap.add_argument("--L3d", type=int, default=5, help="subdivision level of the fem3d k = 3 case")
    a = ap.parse_args()
    run(f"fem2d_P2_L{a.L2d}", m.subdivide(m.fem2d_P2(), a.L2d), 1.5, a.reps)
    run(f"fem3d_k3_L{a.L3d}", m.subdivide(m.fem3d(k=3), a.L3d), 1.5, a.reps)


if __name__ == "__main__":
    main()
