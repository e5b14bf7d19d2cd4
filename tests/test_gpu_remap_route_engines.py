"""Three estimators whose log-polar remaps take different routes alive at once and called in rotation: each engine's remap launches by the
routes it was created with (csrc/mof_kernels.h, SrLpRoute), and each call by its own plan (SrLpPlan).

Resolutions from the default section of tests/golden/sr_lp_route_table.txt, M = 49.9:
  48   staged per 16 x 16 super-tile (SUPER, the 12-deep ring), rows whole dwords apart
  40   staged per wave (WAVE: 40 is no multiple of 16), rows whole dwords apart
  34   res % 4 == 2: staged per wave from rows that are NOT whole dwords apart -- the last image of a batch takes the per-pixel kernel.
       Its batches are dense tensors of exactly n images: nothing of the batch lies behind the last one.
n_images 1 and 3 take the per-pixel kernel, 4 the table-in-LDS kernel at 34 (three staged images are too few) and the staged one at 48 and
40, 5 and 16 the staged one everywhere. Both interpolations. Every output equals the CPU oracle's cv::logPolar bit for bit, and what a
fresh estimator of the same resolution gives when it is the only one."""
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import ScaleRotationEstimator
from mrs_optic_flow_amd.engine import INTER_CUBIC, INTER_LANCZOS4

pytestmark = pytest.mark.gpu
M = 49.9
RESOLUTIONS = (48, 40, 34)
N_IMAGES = (1, 3, 4, 5, 16)
INTERPS = (INTER_CUBIC, INTER_LANCZOS4)


@functools.lru_cache(maxsize=None)
def _images(res):
    """16 images: full-range noise, a smooth ramp under noise, and impulses on black -- read-only"""
    rng = np.random.default_rng(100 + res)
    img = rng.integers(0, 256, (16, res, res), dtype=np.uint8)
    ramp = (np.arange(res)[None, :] * 3 + np.arange(res)[:, None] * 2) % 256
    img[1] = np.clip(ramp + rng.integers(-4, 5, (res, res)), 0, 255)
    img[2] = np.where(rng.random((res, res)) < 0.03, 255, 0)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def _oracle(res, interp):
    """cv::logPolar of every image onto a destination of 7s (pixels mapped from outside the source keep them)"""
    out = np.stack([O.logpolar(im, M, interp, dst=np.full((res, res), 7, np.uint8)) for im in _images(res)])
    out.setflags(write=False)
    return out


def _remap(est, res, n, interp, dev):
    src = torch.tensor(_images(res)[:n], device=dev)  # dense, exactly n images
    dst = torch.full((n, res, res), 7, dtype=torch.uint8, device=dev)
    return est.logpolar_batch_device(src, interp, dst=dst).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _alone(res):
    est = ScaleRotationEstimator(res, M)
    out = {(n, interp): _remap(est, res, n, interp, "cuda:0") for n in N_IMAGES for interp in INTERPS}
    est.close()
    return out


def test_three_estimators_in_rotation(gpu):
    alone = {res: _alone(res) for res in RESOLUTIONS}
    ests = {res: ScaleRotationEstimator(res, M) for res in RESOLUTIONS}
    for n in N_IMAGES:
        for interp in INTERPS:
            for res, est in ests.items():
                got = _remap(est, res, n, interp, gpu)
                assert np.array_equal(got, _oracle(res, interp)[:n]), (res, n, interp, "against the oracle")
                assert np.array_equal(got, alone[res][(n, interp)]), (res, n, interp, "against the estimator used alone")
    for est in ests.values():
        est.close()
