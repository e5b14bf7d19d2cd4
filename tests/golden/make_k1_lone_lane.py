"""Writes tests/golden/k1_lone_lane.npz: the inputs of tests/k1_lone_lane_cases.py and what the library in use computes for every case
on the GPU, bits kept (float64 arrays). Run ONCE from the repository root, with the build the kernels are to be held to -- the commit
before a lone lane handed its pair over, its library named by MOF_LIB_PATH:

    MOF_LIB_PATH=<the parent's libmof_hip.so> python tests/golden/make_k1_lone_lane.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_lone_lane.npz")


def main(path=PATH):
    import torch  # before anything dlopens a HIP runtime

    import k1_lone_lane_cases as L

    g = L.make_inputs()
    L.check_inputs(g)  # the tie cases' exact periods, before anything is recorded
    out = dict(g)
    for name, run in L.CASES:
        got = run(g, torch.device("cuda:0"))
        for key, a in got.items():
            out[f"{name}/{key}"] = np.ascontiguousarray(a, dtype=np.float64)
        s = got["shift"]
        print(f"{name}: {s.shape[0]} pairs x {s.shape[1]} patches, NaN shifts {int(np.isnan(s[..., 0]).sum())}, default == _q bits "
              f"{np.array_equal(got['shift'].view(np.uint64), got['shift_q'].view(np.uint64))}; shifts {np.round(s[:, 0], 2).tolist()}")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, library {os.environ.get('MOF_LIB_PATH', 'the one in the tree')}")


if __name__ == "__main__":
    main(*sys.argv[1:2])
