"""Wall-clock and Newton iterations per second of Zoo problems on the device (the wide path for the vector problems).

    python tools/zoo_bench.py [--repeats R] [case ...]     cases: p_harmonic_fem2d_P2_L7 p_harmonic_fem3d_L4 (default: both)

One untimed solve first (hierarchy upload, plans, analysis), then R timed solves on the same process; prints one JSON
line per case with the median wall-clock, the Newton iterations of a solve and their rate."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mgb_amd as m  # noqa: E402

CASES = {
    "p_harmonic_fem2d_P2_L7": lambda: m.Zoo.p_harmonic(m.amg(m.subdivide(m.fem2d_P2(), 7))),
    "p_harmonic_fem3d_L4": lambda: m.Zoo.p_harmonic(m.amg(m.subdivide(m.fem3d(k=1), 4))),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=list(CASES))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    for name in a.cases:
        t0 = time.perf_counter()
        prob = CASES[name]()
        t_setup = time.perf_counter() - t0
        t0 = time.perf_counter()
        m.mgb_solve(prob)
        t_first = time.perf_counter() - t0
        walls, its = [], 0
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            sol = m.mgb_solve(prob)
            walls.append(time.perf_counter() - t0)
            its = int(sol.SOL_main["its"].sum()) + (int(sol.SOL_feasibility["its"].sum()) if sol.SOL_feasibility else 0)
        wall = statistics.median(walls)
        print(json.dumps(dict(case=name, n=int(prob.M[0].w.size), nD=len(prob.M[0].D_fine), setup_s=round(t_setup, 3),
                              first_solve_s=round(t_first, 3), wall_s=round(wall, 4), newton_its=its,
                              its_per_s=round(its / wall, 1), walls=[round(w, 4) for w in walls])), flush=True)


if __name__ == "__main__":
    main()
