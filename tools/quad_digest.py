"""One SHA-256 per output array of `Quadrature` and `Faces`, for a bitwise A/B of two builds on the same GPU.

`Quadrature`, over the cases of tests/test_gpu_integrate.py with both rules: points, weights, `integrate` for every kind at
p = 1, 1.5, 2, 4 with and without `minus`, totals and element values, `norm(p=inf)` for both kinds; then the shape-edge
geometries of that file (N around G and around the reduction block, Q = 64 and 343, tables staged above 64 KB and read
through L2, 1 / chunk / chunk + 1 columns).  `Faces`, over the TOPOLOGY and WARPED cases of tests/faces_cases.py and the
table-path meshes of tests/test_gpu_faces.py: the four topology arrays, points, normals, measures, interior measures and
face sizes, `integrate` for both kinds with and without `weight`, totals and face values, `jumps` for both kinds and
`indicator`, at p = 1, 1.5, 2, 4 and at 1, 4 and 5 columns.  The summation order is fixed, so two builds that compute the
same thing print the same lines.

Usage: python tools/quad_digest.py [--root DIR] > listing.txt, then cmp two listings.  --root names the checkout whose
package, library and test cases are used (default: the one this file is in), so one copy of the tool can list a build of
another commit.
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.abspath(ap.parse_args().root)
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mgb_amd as m  # noqa: E402
import faces_cases as FC  # noqa: E402
import test_gpu_integrate as GI  # noqa: E402

PS = (1.0, 1.5, 2.0, 4.0)


def line(name, a):
    a = np.ascontiguousarray(a)
    print(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {name} {a.dtype} {a.shape}", flush=True)


def both(name, pair):
    line(name + " total", pair[0])
    line(name + " values", pair[1])


def field(geom, ncol):
    X = geom.xflat
    rng = np.random.default_rng(X.shape[0] + ncol)
    base = np.sin(1.7 * X.sum(axis=1)) + 0.3 * X[:, 0] ** 2
    Z = np.stack([base * (1 + 0.25 * c) + 0.05 * rng.standard_normal(X.shape[0]) + 0.1 * c for c in range(ncol)], axis=1)
    return Z, np.cos(X[:, 0]) + 0.1 * rng.standard_normal(X.shape[0]), rng


def quadrature_calls(what, q, geom, ncol, kinds=("value", "lp", "w1p", "energy"), ps=PS):
    Z, src, rng = field(geom, ncol)
    N, Q, e = q.n_elements, q.n_points, geom.x.shape[2]
    g, G = rng.standard_normal((N, Q, ncol)), rng.standard_normal((N, Q, e))
    for kind in kinds:
        for p in (ps if kind != "value" else (2.0,)):
            kw = dict(source=src) if kind == "energy" else {}
            both(f"{what} {kind} p={p}", q.integrate(Z, kind=kind, p=p, per_element=True, **kw))
            if kind in ("lp", "w1p"):
                both(f"{what} {kind} p={p} minus", q.integrate(Z, kind=kind, p=p, minus=g if kind == "lp" else G, per_element=True))
    if "lp" in kinds:
        line(f"{what} max lp", q.norm(Z, p=np.inf, minus=g))
    if "w1p" in kinds:
        line(f"{what} max w1p", q.norm(Z, p=np.inf, kind="w1p", minus=G))


def quadratures():
    for name in sorted(GI.CASES):
        geom = GI.CASES[name]()
        for rule in ("gauss", "nodal"):
            order = None if rule == "nodal" else GI.ORDERS.get(name)
            with m.Quadrature(geom, order=order, rule=rule) as q:
                what = f"quadrature {name} {rule}"
                line(what + " points", q.points())
                line(what + " weights", q.weights())
                quadrature_calls(what, q, geom, 2)
    G = GI.I.plan(1, 1, 3, 4, 1)["G"]
    B = GI.I.plan(1, 1, 2, 2, 1)["reduce_threads"]
    chunk = GI.I.plan(2, 2, 7, 16, 8)["chunk"]
    edges = [(f"interval_N{N}", GI._interval(N), 4, 1) for N in (1, G - 1, G, G + 1)]
    edges += [(f"interval_k1_N{N}", GI._interval(N, k=1), 2, 1) for N in (B - 1, B, B + 1)]
    edges += [("fem3d_k1_n4", GI._fem3d(1, 5), 4, 1), ("fem3d_k1_n7", GI._fem3d(1, 2), 7, 1), ("fem3d_k3_n4", GI._fem3d(3, 5), 4, 1),
              ("fem3d_k4_n5", GI._fem3d(4, 1), 5, 1)]
    edges += [(f"fem2d_P2_ncol{n}", GI.CASES["fem2d_P2"](), None, n) for n in (1, chunk, chunk + 1)]
    for name, geom, order, ncol in edges:
        with m.Quadrature(geom, order=order) as q:
            quadrature_calls(f"quadrature edge {name}", q, geom, ncol, ps=(1.5, 4.0))


def face_calls(what, fc, geom, ncols=(1, 4, 5), ps=PS):
    rng = np.random.default_rng(5)
    W = rng.standard_normal((fc.n_boundary, fc.n_points))
    for ncol in ncols:
        Z = FC.broken_field(geom, ncol=ncol)
        tag = f"{what} ncol={ncol}"
        both(tag + " value", fc.integrate(Z, kind="value", per_face=True))
        both(tag + " value weight", fc.integrate(Z, kind="value", weight=W, per_face=True))
        line(tag + " jumps value", fc.jumps(Z, kind="value"))
        for p in ps:
            both(f"{tag} flux p={p}", fc.integrate(Z, kind="flux", p=p, per_face=True))
            both(f"{tag} flux p={p} weight", fc.integrate(Z, kind="flux", p=p, weight=W, per_face=True))
            line(f"{tag} jumps flux p={p}", fc.jumps(Z, kind="flux", p=p))
            eta2, total = fc.indicator(Z, p=p)
            line(f"{tag} indicator p={p} eta2", eta2)
            line(f"{tag} indicator p={p} total", total)


def faces():
    meshes = [(f"topology {name}", FC.TOPOLOGY[name], None) for name in sorted(FC.TOPOLOGY)]
    meshes += [(f"warped {name}",) + FC.WARPED[name] for name in sorted(FC.WARPED)]
    q3 = lambda: m.fem3d(k=3, K=FC.warp(FC.pair(3, 3, np.eye(3)).x, 0.03))                # tests/test_gpu_faces.py: the table paths
    meshes += [("q3 pair order 3", q3, 3), ("q3 pair order 4", q3, 4),
               ("p1 L4", lambda: m.fem2d_P1(K=FC.warp(m.subdivide(m.fem2d_P1(), 4).x)), 2)]
    for what, fn, order in meshes:
        geom = fn()
        with m.Faces(geom, order=order) as fc:
            what = "faces " + what
            for f in ("boundary", "interior", "orientation", "element_faces"):
                line(f"{what} {f}", getattr(fc, f))
            for f in ("points", "normals", "measures", "interior_measures", "face_sizes"):
                line(f"{what} {f}", getattr(fc, f)())
            if what.startswith("faces q3"):
                face_calls(what, fc, geom, ncols=(1,), ps=(1.5,))
            else:
                face_calls(what, fc, geom)


if __name__ == "__main__":
    quadratures()
    faces()
