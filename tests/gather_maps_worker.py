"""Worker of tests/test_gpu_gather_maps.py (the solver's switches are read once per process): one whole solve of fem2d_P2,
p = 1.0 at refinement L through mgb_driver; writes z, the Newton iterations and the fine level's factorization launches.

python gather_maps_worker.py OUT.npz L"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(out, L):
    sys.path.insert(0, ROOT)
    import mgb_amd as m
    from mgb_amd.device import DeviceMGBProblem
    from mgb_amd.solve import mgb_driver
    prob = m.assemble(m.amg(m.subdivide(m.fem2d_P2(), L), prolongator=m.amg_ruge_stuben()), p=1.0)
    D = DeviceMGBProblem(prob, device_id=0)
    SOL = mgb_driver(D)
    fine = len(D.main.level_sizes) - 1
    rows = D.main.solver_launches(fine)
    np.savez(out, z=SOL["z"], its=np.asarray(SOL["SOL_main"]["its"]), rows=np.array(json.dumps(rows)))
    D.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
