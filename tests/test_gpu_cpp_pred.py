"""GPU test of the C++ mirror of the window-offset entries (include/mof/processors.hpp: reservePred, processBatchDevicePred,
processCoarseToFineBatchDevice, processImageCoarseToFine) through tests/cpp/test_pred: the driver compares each method with the C ABI
entry it mirrors, byte for byte, and prints every value; here they are compared with the Python binding's bits."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pred_cases as PC
from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "test_pred")


def test_cpp_mirror_has_the_c_abis_bits(gpu, tmp_path):
    assert os.path.exists(BIN), "tests/cpp/test_pred missing: run __graft_entry__.build()"
    l, cur, prev, _, _ = PC.c2f_case(128)
    px, py = 21, -18  # (not what the long-range pass predicts: the two batch entries must differ)
    path = tmp_path / "pairs.u8"
    np.concatenate([cur, prev]).tofile(path)
    r = subprocess.run([BIN, "128", "32", repr(PC.SPEED), str(px), str(py), "2", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [line.split() for line in r.stdout.strip().split("\n")]
    assert lines[-1] == ["abi", "same"], lines[-1]
    rows = {(t[0], int(t[1])): t[2:] for t in lines[:-1]}
    fm = FftMethod(128, 32, PC.SPEED)
    tc, tp = torch.tensor(cur, device=gpu), torch.tensor(prev, device=gpu)
    pred = torch.tensor(np.broadcast_to(np.array([px, py], np.int32), (2, 16, 2)).copy(), device=gpu)
    out, q, a = (t.cpu().numpy() for t in fm.process_batch_device_pred(tc, tp, pred, return_quality=True, return_applied=True))
    cout, ca, coarse = (t.cpu().numpy() for t in fm.process_coarse_to_fine_batch_device(tc, tp, return_applied=True, return_coarse=True))
    assert not np.array_equal(a, ca)

    def bits(v):
        return np.ascontiguousarray(v, np.float64).view(np.uint64)

    for k in range(2):
        got = np.array([float(v) for v in rows[("pred", k)]]).reshape(16, 6)
        assert np.array_equal(bits(got[:, :2]), bits(out[k])) and np.array_equal(bits(got[:, 2:4]), bits(q[k]))
        assert np.array_equal(got[:, 4:].astype(np.int64), a[k])
        got = np.array([float(v) for v in rows[("c2f", k)]]).reshape(16, 4)
        assert np.array_equal(bits(got[:, :2]), bits(cout[k])) and np.array_equal(got[:, 2:].astype(np.int64), ca[k])
        assert np.array_equal(bits(np.array([float(v) for v in rows[("coarse", k)]]).reshape(1, 2)), bits(coarse[k]))
        # the stateful method: previous then current of the pair = the batch entry's pair
        tok = rows[("image", k)]
        assert tok[0] == "invalid" and int(tok[1]) == int(np.isnan(cout[k][:, 0]).sum())
        assert np.array_equal(bits(np.array([float(v) for v in tok[2:]]).reshape(16, 2)), bits(cout[k]))
