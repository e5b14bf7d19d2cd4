"""Writes tests/golden/k1_finish.npz: the inputs of tests/k1_finish_cases.py and what the library in use computes for every case on
the GPU, bits kept (float64 arrays). Run ONCE from the repository root, with the build the kernels are to be held to (the commit before
the wave that holds the maximum ended the patch):

    python tests/golden/make_k1_finish.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "k1_finish.npz")


def main(path=PATH):
    import torch  # before anything dlopens a HIP runtime

    import k1_finish_cases as K

    g = K.make_inputs()
    out = dict(g)
    for name, run in K.CASES:
        got = run(g, torch.device("cuda:0"))
        for key, a in got.items():
            out[f"{name}/{key}"] = np.ascontiguousarray(a, dtype=np.float64)
        s = got["shift"]
        print(f"{name}: {s.shape[0]} pairs x {s.shape[1]} patches, NaN shifts {int(np.isnan(s[..., 0]).sum())}, default == _q bits "
              f"{np.array_equal(got['shift'].view(np.uint64), got['shift_q'].view(np.uint64))}; shifts {np.round(s[:, 0], 2).tolist()}")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(*sys.argv[1:2])
