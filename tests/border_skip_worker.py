"""Worker of tests/test_gpu_border_skip.py (the solver's switches are read once per process).

python border_skip_worker.py OUT.npz ladder L     every level of the fem2d_P2 (p = 1.0) hierarchy at refinement L: two Newton
                                                  directions formed as the resident loop forms them (mgbhip_newton_direction; the
                                                  second one factors again, from condensed leaves where the level has them), then a
                                                  generic factor + solve of the same Hessian, and the level's launch rows
python border_skip_worker.py OUT.npz reject TAG [TAG ...]
                                                  tests/solver_gate_cases.py: the zero-pivot matrix of TAG through the carried path
                                                  (rejected: the status word says so), then the case's regular matrix through it"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ladder(out, L):
    import mgb_amd as m
    from mgb_amd import device as dev
    from mgb_amd.device import DeviceMGBProblem
    prob = m.assemble(m.amg(m.subdivide(m.fem2d_P2(), L), prolongator=m.amg_ruge_stuben()), p=1.0)
    D = DeviceMGBProblem(prob, device_id=0)
    P = D.main
    z0 = np.ascontiguousarray(prob.g.T).reshape(-1)
    c = 0.1 * prob.f
    res = {"levels": np.array(len(P.level_sizes))}
    for J in range(len(P.level_sizes)):
        s = np.zeros(P.level_sizes[J])
        for rep in ("a", "b"):
            try:
                x, lam, cond = P.newton_direction(J, s, c, z0)
                status = 0.0
            except dev.MGBHipError as e:
                x, lam, cond, status = np.full(s.size, np.nan), np.nan, False, float(e.status)
            res[f"l{J}_x{rep}"], res[f"l{J}_lam{rep}"] = x, np.array([lam, status, float(cond)])
        g = P.f1(J, s, c, z0)
        P.f2(J, s, c, z0)
        res[f"l{J}_xg"] = P.solve(J, g)                 # generic: identity border, forward and backward sweep
        x, lam, cond = P.newton_direction(J, s, c, z0)  # and the carried path once more after it
        res[f"l{J}_xc"], res[f"l{J}_lamc"] = x, np.array([lam, 0.0, float(cond)])
        res[f"l{J}_rows"] = np.array(json.dumps(P.solver_launches(J)))
    D.close()
    np.savez(out, **res)


def reject(out, tags):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import solver_gate_cases as S
    from mgb_amd.device import DeviceProblem, HipContext
    prob = S.problem()
    ctx = HipContext(0)
    P = DeviceProblem(ctx, prob.M[0], prob.Q)
    res = {}
    for tag in tags:
        name = S.ZERO[tag][1]
        lev = S.LEVEL[name]
        A0, g0, _, _ = S.zero_pivot_system(tag)
        A, g, _ = S.system(name, 0)
        P.set_hessian(lev, A0.data)
        x, lam, status = P.solve_newton(lev, g0, check=False)
        res[tag + "_zero_x"], res[tag + "_zero"] = x, np.array([lam, float(status)])
        for rep in ("", "_again"):
            P.set_hessian(lev, A.data)
            x, lam, status = P.solve_newton(lev, g, check=False)
            res[tag + "_x" + rep], res[tag + "_lam" + rep] = x, np.array([lam, float(status)])
        P.set_hessian(lev, A.data)
        res[tag + "_xg"] = P.solve(lev, g)
        res[tag + "_rows"] = np.array(json.dumps(P.solver_launches(lev)))
    P.close()
    ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if sys.argv[2] == "ladder":
        ladder(sys.argv[1], int(sys.argv[3]))
    else:
        reject(sys.argv[1], sys.argv[3:])
