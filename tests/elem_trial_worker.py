"""Worker of tests/test_gpu_elem.py for the switches the library reads once per process (MGBHIP_NO_FUSED_STEP,
MGBHIP_NO_FUSED_RESTRICT, MGBHIP_NO_PACKED_LEAVES; the caller sets them in the environment).

python elem_trial_worker.py OUT.npz trial CASE       the line-search trial of an elem_cases problem at its finest level
python elem_trial_worker.py OUT.npz condense MESH    two Newton directions on a fem2d_P2 mesh (test_gpu_elem.condense_problem)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main(out, what, name):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    if what == "trial":
        import elem_cases as E
        from test_gpu_elem import open_case
        ctx, P = open_case(name)
        b = E.built(name)
        s, c, z0 = E.inputs(name, 1)
        t = P.trial_values(1, s, b.dirs[1], E.TRIAL_STEP, c, z0)
        plan = P.elem_plan("f01")
        np.savez(out, y=t["y"], g=t["g"], xn=t["xn"], flags=np.array([t["moved"], t["finite"], t["on_the_fly"], t["fused_restrict"]]),
                 plan=json.dumps(plan))
    else:
        from test_gpu_elem import condense_problem, condense_run
        np.savez(out, **condense_run(condense_problem(name)))


if __name__ == "__main__":
    main(*sys.argv[1:4])
