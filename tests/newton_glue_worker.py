"""Worker of tests/test_gpu_newton_glue.py.  MGBHIP_FINISH_SERIAL, MGBHIP_SPLIT_START and MGBHIP_Z_SNAPSHOT are read once per
process, so every path runs in a process of its own: this script runs the named parts under the environment it is given
and writes everything it computed into one .npz file.

python newton_glue_worker.py OUT.npz PART [PART ...]        PART: solves | edges | record | levels | reject | snapshot"""
import math
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SWITCHES = ("MGBHIP_FINISH_SERIAL", "MGBHIP_SPLIT_START", "MGBHIP_Z_SNAPSHOT")
# the paths before this change, each new path alone, and all three together
CONFIGS = {
    "old": SWITCHES,
    "finish": ("MGBHIP_SPLIT_START", "MGBHIP_Z_SNAPSHOT"),
    "start": ("MGBHIP_FINISH_SERIAL", "MGBHIP_Z_SNAPSHOT"),
    "snapshot": ("MGBHIP_FINISH_SERIAL", "MGBHIP_SPLIT_START"),
    "new": (),
}
SOLVES = ("p2_L3_p1", "p2_L3_p15", "fem1d", "fem3d", "phase1", "spectral", "fem1d_illinois")
DIAG = ("its", "ts", "kappas", "c_dot_Dz", "newton_iterations", "f0_evals", "f1_evals", "f2_evals", "factorizations", "k", "t_final")


def finish_loads_in_flight():
    """U of finish_kernel<U> (csrc/reduce_kernels.hpp): partials per job and thread requested before the first addition."""
    src = open(os.path.join(ROOT, "multigridbarrier.jl_amd", "csrc", "reduce_kernels.hpp")).read()
    return int(re.search(r"constexpr int FINISH_LOADS_IN_FLIGHT = (\d+);", src).group(1))


EPB = 128                     # elements per workgroup of the fem1d element kernels (two lanes per element, 256 threads)


def edge_elements():
    """Elements N of single-level fem1d problems (m = 3 N - 1 unknowns): the count of f0 partials, ceil(N / 128), takes the values
    1, 255, 256, 257, 256 U - 1, 256 U, 256 U + 1 and 3 * 256 U + 5; the workgroups of a vector reduction, min(ceil(m / 256), cap),
    the values 1, 2, 1023 (= cap - 1) and 1024 (the cap, here by the cap itself)."""
    U = finish_loads_in_flight()
    counts = [255, 256, 256 * U - 1, 256 * U, 3 * 256 * U + 5]
    return [64, 128] + [c * EPB for c in counts] + [256 * EPB + 1, 256 * U * EPB + 1, 87296, 87424]


DIRECTION_N = (64, 128, 87296, 87424)      # a Newton direction factors the level: only where that stays quick


def edge_inputs(N):
    cu, n = N - 1, 2 * N
    t = (np.arange(cu) + 1.0) / (cu + 1.0)
    j = np.arange(n)
    s = 1e-3 * np.concatenate([np.sin(math.pi * t) * (1.0 + 0.5 * np.cos(5.0 * t)), np.cos(0.7 * j) + 0.3 * np.sin(0.01 * j + 1.0)])
    d = 1e-3 * np.concatenate([np.sin(2.0 * math.pi * t), np.sin(0.3 * j) - 0.2])
    return s, d


# (gate case, level): a level with columns <= 64 (thread per row), two wave-per-row levels, the chunked restriction on both
# sides of its gate (1023 / 1024 entries in the longest column), three chunks, and the selection level
START_LEVELS = (("restrict_cols", 1), ("restrict_cols", 2), ("restrict_cols", 3), ("restrict_cols", 4), ("restrict_cols", 0),
                ("restrict_cols", 9), ("prolong_rows", 1))


def _problem(name):
    import mgb_amd as m
    from helpers import literal_fem1d_problem
    if name in ("p2_L3_p1", "p2_L3_p15"):
        return m.assemble(m.amg(m.subdivide(m.fem2d_P2(), 3)), p=1.0 if name == "p2_L3_p1" else 1.5)
    if name in ("fem1d", "fem1d_illinois"):
        return m.assemble(m.amg(m.fem1d(nodes=np.linspace(-1, 1, 9))), p=1.5)
    if name == "fem3d":
        return m.assemble(m.amg(m.subdivide(m.fem3d(k=1), 2)), p=1.5)
    if name == "spectral":                      # 100 nodes > 64: the dense path
        return m.assemble(m.amg(m.spectral2d(n=10)), p=1.5)
    if name == "phase1":                        # the start violates the cone on the long element: phase I runs first
        prob = literal_fem1d_problem((-1.0, 0.25, 1.0), 1.5)
        prob.g[:, 1] = 0.5
        return prob
    raise KeyError(name)


def _keep(out, tag, diag):
    for k in DIAG:
        out[f"{tag}/{k}"] = np.asarray(diag[k])
    out[f"{tag}/z"] = np.asarray(diag["z"])


def part_solves(out):
    from mgb_amd.device import DeviceMGBProblem
    from mgb_amd.solve import mgb_driver
    for name in SOLVES:
        D = DeviceMGBProblem(_problem(name), device_id=0)
        SOL = mgb_driver(D, **(dict(line_search=("illinois",)) if name == "fem1d_illinois" else {}))
        D.close()
        _keep(out, f"solve/{name}/main", SOL["SOL_main"])
        out[f"solve/{name}/phase1"] = np.array(SOL["SOL_feasibility"] is not None)
        if SOL["SOL_feasibility"] is not None:
            _keep(out, f"solve/{name}/feas", SOL["SOL_feasibility"])


def part_edges(out):
    import gate_cases as G
    from mgb_amd.device import DeviceProblem, HipContext
    ctx = HipContext(0)
    for N in edge_elements():
        prob = G.fem1d_problem(N, [])
        P = DeviceProblem(ctx, prob.M[0], prob.Q)
        s, d = edge_inputs(N)
        c, z0 = 0.1 * prob.f, np.ascontiguousarray(prob.g.T).reshape(-1)
        out[f"edge/{N}/grid"] = np.array(P.elem_plan("f01")["grid"])
        out[f"edge/{N}/m"] = np.array(P.level_sizes[0])
        out[f"edge/{N}/f0"] = np.array(P.f0(0, s, c, z0))
        t = P.trial_values(0, s, d, 0.5, c, z0)
        out[f"edge/{N}/trial_y"] = np.array(t["y"])
        out[f"edge/{N}/trial_g"] = t["g"]
        out[f"edge/{N}/trial_flags"] = np.array([t["moved"], t["finite"]])
        if N in DIRECTION_N:
            x, lam, _ = P.newton_direction(0, s, c, z0)
            out[f"edge/{N}/dir_x"] = x
            out[f"edge/{N}/dir_lambda2"] = np.array(lam)
        P.close()
    ctx.close()


class Recorder:
    """The default stopping rule (stopping_inexact with the library's own constants) as a callable that keeps every
    argument it is given: ymin and gmin of a Newton solve's first call are the start point's y and |g|."""

    def __init__(self, P):
        o = P.default_options()
        self.lambda_tol, self.theta = o.stop_lambda_tol, o.stop_theta
        self.rows = []
        self.blocked = -1                   # after block(): no, yes, and then always no (counts the calls since)
        self.said_yes = False

    def block(self):
        self.blocked = max(self.blocked, 0)

    def __call__(self, ymin, ynext, gmin, gnext, n, ndecmin, ndec):
        gn = float(gnext[0])
        self.rows.append((ymin, ynext, gmin, gn, ndecmin, ndec))
        if self.blocked >= 0:
            self.blocked += 1
            self.said_yes = self.said_yes or self.blocked == 2
            return self.blocked == 2
        return (ndec < self.lambda_tol) or (ynext >= ymin and gn >= self.theta * gmin)


def part_record(out):
    """Whole solves under the recording rule: the fem2d_P2 ladder (selection fine level, projected coarse levels) and the gate
    suite's solve hierarchy with one Newton iteration per level attempt, so that the attempts recurse into the level with the
    chunked restriction (its first four t-steps)."""
    import gate_cases as G
    from mgb_amd.device import DeviceMGBProblem
    from mgb_amd.solve import MGBConvergenceFailure, mgb_driver
    for name, prob, kw, steps in (("p2_L3_p1", _problem("p2_L3_p1"), {}, 1000), ("gate_solve", G.solve_problem(), dict(max_newton=1), 4)):
        D = DeviceMGBProblem(prob, device_id=0)
        rec = Recorder(D.main)
        zs = []

        def seen(z, t):                      # early_stop: ends the ramp after `steps` t-steps
            zs.append(np.array(z, copy=True))
            return len(zs) >= steps
        try:
            mgb_driver(D, stopping_criterion=rec, early_stop=seen, **kw)
            out[f"record/{name}/failed"] = np.array(False)
        except MGBConvergenceFailure:
            out[f"record/{name}/failed"] = np.array(True)
        D.close()
        out[f"record/{name}/calls"] = np.array(rec.rows)
        out[f"record/{name}/z"] = np.array(zs)


def part_levels(out):
    """Run with MGBHIP_NO_FUSED_STEP=1 MGBHIP_NO_FUSED_RESTRICT=1: a trial with step 0 is then the launch sequence of the Newton
    start (the f01 element kernel at a stored point, eval_f1's restriction, block_reduce<1>, one finishing launch)."""
    import gate_cases as G
    from mgb_amd.device import DeviceProblem, HipContext
    ctx = HipContext(0)
    held = {}
    for name, level in START_LEVELS:
        if name not in held:
            prob = G.problem(name)
            held[name] = DeviceProblem(ctx, prob.M[0], prob.Q)
        P = held[name]
        s, c, z0 = G.inputs(name, level)
        tag = f"level/{name}/{level}"
        out[f"{tag}/plan"] = np.array([P.level_plan(level)[k] for k in ("R_unit", "T_long", "T_chunks")], dtype=np.int64)
        out[f"{tag}/f0"] = np.array(P.f0(level, s, c, z0))
        out[f"{tag}/f1"] = P.f1(level, s, c, z0)
        t = P.trial_values(level, s, np.zeros_like(s), 0.0, c, z0)
        out[f"{tag}/trial_y"] = np.array(t["y"])
        out[f"{tag}/trial_g"] = t["g"]
        out[f"{tag}/trial_x"] = t["xn"] - s
        out[f"{tag}/path"] = np.array([t["on_the_fly"], t["fused_restrict"], t["finite"]], dtype=np.int64)
    for P in held.values():
        P.close()
    ctx.close()


def _main_options(D, **kw):
    """What mgb_driver hands the main phase, for calling mgb_core directly (its result survives a failed solve)."""
    from mgb_amd.solve import _barrier_weights, _options
    M1 = D.prob.M[0]
    D.main.set_barrier_weights(_barrier_weights(M1.w, M1.w != 0))
    keep = []
    a = dict(tol=None, t=0.1, kappa=None, maxit=None, max_newton=None, line_search=None, stopping_criterion=None, finalize=None,
             early_stop=0, keep=keep)
    a.update(kw)
    return _options(D.main, **a), keep


def part_reject(out):
    """An infeasible start (slack 0.5 < |u'| = 1) is rejected with the start point's message; the next solve on the same
    handle is the ordinary one."""
    from helpers import stacked
    from mgb_amd.device import DeviceMGBProblem, MGBHipError
    prob = _problem("fem1d")
    D = DeviceMGBProblem(prob, device_id=0)
    opt, keep = _main_options(D)
    bad = prob.g.copy()
    bad[:, 1] = 0.5
    try:
        D.main.mgb_core(stacked(bad), prob.f, opt)
        msg = "no error"
    except MGBHipError as e:
        msg = str(e)
    out["reject/message"] = np.array(msg)
    status, z, diag = D.main.mgb_core(stacked(prob.g), prob.f, opt)
    diag["z"] = z
    out["reject/status"] = np.array(status)
    _keep(out, "reject/next", diag)
    D.close()


def part_snapshot(out):
    """fem2d_P2 L = 2 with one Newton iteration per level attempt: every t-step's first attempt (all levels at once) fails and
    recurses, and the second t-step fails seven times (kappa 10 -> 10^(1/128)) before it is accepted.
    a) that solve, ended by maxit = 8;
    b) the same, but once the ramp has started the rule says no to the first level solve (all levels at once), yes to the
       second (the coarse half of the recursion, whose result is prolonged into z) and no ever after: every t-step fails
       and is rolled back until kappa reaches 1.  early_stop sees z when the ramp starts and again when it has given up."""
    import mgb_amd as m
    from helpers import stacked
    from mgb_amd.device import DeviceMGBProblem
    prob = m.assemble(m.amg(m.subdivide(m.fem2d_P2(), 2)), p=1.0)
    D = DeviceMGBProblem(prob, device_id=0)
    opt, keep = _main_options(D, max_newton=1, maxit=8)
    status, z, diag = D.main.mgb_core(stacked(prob.g), prob.f, opt)
    diag["z"] = z
    out["snapshot/recurse/status"] = np.array(status)
    _keep(out, "snapshot/recurse", diag)
    D.close()

    D = DeviceMGBProblem(prob, device_id=0)
    rec = Recorder(D.main)
    zs = []

    def seen(z, t):
        zs.append(np.array(z, copy=True))
        rec.block()
        return False
    opt, keep = _main_options(D, max_newton=1, stopping_criterion=rec, early_stop_fn=seen)
    status, z, diag = D.main.mgb_core(stacked(prob.g), prob.f, opt)
    diag["z"] = z
    out["snapshot/rollback/status"] = np.array(status)
    out["snapshot/rollback/failure_code"] = np.array(diag["failure_code"])
    out["snapshot/rollback/said_yes"] = np.array(rec.said_yes)
    out["snapshot/rollback/seen"] = np.array(zs)
    _keep(out, "snapshot/rollback", diag)
    D.close()


PARTS = dict(solves=part_solves, edges=part_edges, record=part_record, levels=part_levels, reject=part_reject, snapshot=part_snapshot)


def main(path, parts):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    out = {}
    for p in parts:
        PARTS[p](out)
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2:])
