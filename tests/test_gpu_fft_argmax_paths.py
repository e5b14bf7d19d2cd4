"""K1's arg-max reduces the VALUE first (a wave maximum, then the workgroup's) and walks the (value, index) chain only in a wave that
holds the maximum (csrc/pc_kernel.hip, csrc/pc_argmax.hpp). The result has to be the Best the pair fold gave before, bit for bit. The
fixtures tests/golden/argmax_paths_n*.npz (made by tests/golden/make_argmax_paths.py, which describes them) put the peak into every
wave's columns, both packed halves and every row residue, and add periodic textures whose surface attains its maximum several times --
in one lane, across lanes, across waves --, one constant pair and one pair with a constant prev. The expected shifts and quality were
recorded ONCE on the GPU from the commit before the value-first arg-max; every float64 must come out with the same bits, through the
default entry and through the _q entry. (An exact tie cannot be forced from outside: tests/cpp/test_argmax_select.cpp carries that.)"""
import os

import numpy as np
import pytest
import torch

from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("n", [64, 32])
def test_same_bits_as_the_pair_fold(gpu, n):
    g = np.load(os.path.join(GOLDEN, f"argmax_paths_n{n}.npz"))
    fm = FftMethod(sample_point_size=n, frame_shape=(n, n), grid=(1, 1))
    tc, tp = torch.from_numpy(g["cur"]).to(gpu), torch.from_numpy(g["prev"]).to(gpu)
    got = fm.process_batch_device(tc, tp).cpu().numpy()[:, 0]
    s, q = fm.process_batch_device(tc, tp, return_quality=True)
    got_q, qual = s.cpu().numpy()[:, 0], q.cpu().numpy()[:, 0]
    names = g["names"]
    for what, have, want in (("default entry", got, g["want_shift"]), ("_q entry, shift", got_q, g["want_shift_q"]),
                             ("_q entry, quality", qual, g["want_quality"])):
        bad = np.nonzero((_bits(have) != _bits(want)).any(axis=1))[0]
        for k in bad:
            print(f"argmax paths n={n} {what} [{names[k]}]: got {have[k].tolist()} recorded {want[k].tolist()}")
        assert len(bad) == 0, (n, what, [str(names[k]) for k in bad])
    # the sweep returns what was planted, to within the sample (the record is not NaN throughout by accident): every pair but the 18
    # whose peak sits in shifted row or column 0 -- there the clamped window pulls the centroid past -n/2 and the gate answers NaN
    sweep = ~np.isnan(g["planted"][:, 0])
    valid = sweep & ~np.isnan(got[:, 0])
    assert sweep.sum() == 90 and valid.sum() == 72 and np.abs(got[valid] - g["planted"][valid]).max() < 0.5
