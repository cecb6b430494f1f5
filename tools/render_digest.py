"""One SHA-256 per output array of the rendering family, for a bitwise A/B of two builds on the same GPU.

Covers trace (max_hits 1, 4, 8), shade and render over the GPU cases of tests/test_surface.py, tests/test_tubes.py and
tests/test_raycast.py (render with and without layers), and one `FigureRenderer` frame per geometry of
tests/test_gpu_figure.py, with and without the volume, 32 x 24.  With contraction off and the order of operations
kept, IEEE arithmetic leaves no room: two builds that compute the same thing print the same lines.

Usage: python tools/render_digest.py [--root DIR] > listing.txt, then diff two listings.  --root names the checkout
whose package, library and test cases are used (default: the one this file is in), so one copy of the tool can list a
build of another commit.
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
import test_raycast as RC  # noqa: E402
import test_surface as SF  # noqa: E402
import test_tubes as TB  # noqa: E402
from mgb_amd.raycast import _diagonal, clip_box  # noqa: E402

AMBIENT = 0.3
EYE, TARGET = (2.7, -3.1, 1.9), (0.0, 0.0, 0.0)


def line(name, a):
    a = np.ascontiguousarray(a)
    print(f"{hashlib.sha256(a.tobytes()).hexdigest()}  {name} {a.dtype} {a.shape}", flush=True)


def table():
    t = RC.TABLE5.copy()
    t[:, 3] = [0.0, 0.7, 1.3, 0.4, 1.0]
    return t


def surfaces():
    for name in sorted(SF.GPU_CASES):
        pts, o, d, t_min, t_max, _ = SF.case_soup(name)
        with m.TriangleCaster(pts) as tc:
            for K in (1, 4, 8):
                h = tc.trace(o, d, t_min, t_max, max_hits=K)
                for f in ("t", "triangle", "u", "v"):
                    line(f"surface {name} trace K={K} {f}", getattr(h, f))
                line(f"surface {name} shade K={K}", tc.shade(h, d, SF.vertex_values(pts), table(), RC.CLIM, AMBIENT))


def tubes():
    for name in sorted(TB.GPU_CASES):
        pts, rad, o, d, t_min, t_max = TB.case_tubes(name)
        with m.SegmentCaster(pts, rad) as sc:
            for K in (1, 4, 8):
                h = sc.trace(o, d, t_min, t_max, max_hits=K)
                for f in ("t", "segment", "s"):
                    line(f"tubes {name} trace K={K} {f}", getattr(h, f))
                line(f"tubes {name} shade K={K}", sc.shade(h, o, d, TB.end_values(pts), table(), RC.CLIM, AMBIENT))


def volumes():
    for name in sorted(RC.GPU_CASES):
        make, rays, step, t_min, t_max = RC.GPU_CASES[name]
        geom = make()
        o, d = rays()
        u = RC.smooth(geom.xflat)[:, 0]
        R = o.shape[0]
        depth = np.sort(np.linspace(0.3, 3.9, R * 2).reshape(R, 2), axis=1)
        depth[::3, 1] = np.inf                                    # a missing second layer on every third ray
        layers = 0.25 + 0.5 * np.abs(np.sin(np.arange(R * 2 * 4, dtype=np.float64))).reshape(R, 2, 4)
        with m.RayCaster(geom, o, d, step, t_min=t_min, t_max=t_max) as rc:
            line(f"raycast {name} offsets", rc.offsets)
            line(f"raycast {name} render", rc.render(u, RC.TABLE5, RC.CLIM))
            if o.shape[1] == 3:                                   # layers need a 3-D mesh
                line(f"raycast {name} render layers", rc.render(u, RC.TABLE5, RC.CLIM, layers=(depth, layers)))


def figures():
    geoms = {"k1x64": SF.sphere_geom, "k2x8": lambda: m.subdivide(m.fem3d(k=2), 1)}       # tests/test_gpu_figure.py
    for name in sorted(geoms):
        geom = geoms[name]()
        u = np.ascontiguousarray(RC.smooth(geom.xflat)[:, 0])
        for volume in (True, False):
            with m.FigureRenderer(geom, EYE, TARGET, size=(32, 24), isosurfaces=[-0.35, 0.2, 0.61, 1.1], clim=(-1.0, 3.0),
                                  slices=[(0, 0.25), (2, -0.1)], volume=volume, surface_alpha=0.6,
                                  step=_diagonal(clip_box(geom)) / 16.0, ambient=0.25) as fr:
                what = f"figure {name} {'volume' if volume else 'surfaces'}"
                line(what + " frame", fr.render(u))
                line(what + " rgba8", fr.render_rgba8(u, (0.1, 0.45, 0.8)))


if __name__ == "__main__":
    surfaces()
    tubes()
    volumes()
    figures()
