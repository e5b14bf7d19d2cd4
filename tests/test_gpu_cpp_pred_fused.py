"""GPU test of the C++ mirror of the fused window-offset route (include/mof/processors.hpp: setPredRoute, predRoute,
processBatchDevicePredBgr, and processBatchDevicePred on that route) through tests/cpp/test_pred_fused: the driver compares each method
with the C ABI entry it mirrors, byte for byte, and prints every value; here they are compared with the Python binding's bits."""
import os
import subprocess

import numpy as np
import pytest
import torch

import pred_cases as PC
import pred_fused_cases as F
from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
BIN = os.path.join(os.path.dirname(__file__), "cpp", "test_pred_fused")


def test_cpp_mirror_of_the_fused_route_has_the_c_abis_bits(gpu, tmp_path):
    assert os.path.exists(BIN), "tests/cpp/test_pred_fused missing: run __graft_entry__.build()"
    l, cur, prev, _, _ = PC.c2f_case(128)
    px, py = 21, -18
    path = tmp_path / "pairs.u8"
    np.concatenate([cur, prev]).tofile(path)
    r = subprocess.run([BIN, "128", "32", repr(PC.SPEED), str(px), str(py), "2", str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = [line.split() for line in r.stdout.strip().split("\n")]
    assert lines[-1] == ["abi", "same"], lines[-1]
    assert lines[-2] == ["refused", "bgr-on-gather", "route-2"], lines[-2]
    rows = {(t[0], int(t[1])): t[2:] for t in lines[:-2]}
    fm = FftMethod(128, 32, PC.SPEED)
    fm.set_pred_route("fused")
    pred = torch.tensor(np.broadcast_to(np.array([px, py], np.int32), (2, 16, 2)).copy(), device=gpu)
    gray = [t.cpu().numpy() for t in fm.process_batch_device_pred(torch.tensor(cur, device=gpu), torch.tensor(prev, device=gpu), pred,
                                                                  return_quality=True, return_applied=True)]
    bgr = [t.cpu().numpy() for t in fm.process_batch_device_pred_bgr(torch.tensor(F.bgr_of(cur), device=gpu), torch.tensor(F.bgr_of(prev), device=gpu),
                                                                     pred, return_quality=True, return_applied=True)]

    def bits(v):
        return np.ascontiguousarray(v, np.float64).view(np.uint64)

    assert not np.array_equal(bits(gray[0]), bits(bgr[0]))  # (the channels differ: the two entries see different pixels)
    for tag, (out, q, a) in (("pred", gray), ("bgr", bgr)):
        for k in range(2):
            got = np.array([float(v) for v in rows[(tag, k)]]).reshape(16, 6)
            assert np.array_equal(bits(got[:, :2]), bits(out[k])) and np.array_equal(bits(got[:, 2:4]), bits(q[k])), (tag, k)
            assert np.array_equal(got[:, 4:].astype(np.int64), a[k]), (tag, k)
