"""GPU tests of the kernel forms that are NOT the default route (A/B knobs): each must pass the parity tests of the form it
replaces -- remap ring / super-tile / staged forms. (Forms whose A/B is closed are not kept correct here: they leave the library,
docs/history/retired_switches.md.)"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_REMAP_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np, torch
import oracle_lib as O, sr_scenes
from mrs_optic_flow_amd import ScaleRotationEstimator
from mrs_optic_flow_amd.engine import INTER_CUBIC, INTER_LANCZOS4
dev = torch.device("cuda", 0)
checked = 0
for res, M in ((480, 49.9), (256, 45.0)):
    base = sr_scenes.canvas(900 + res, res)
    frames = np.stack([sr_scenes.view(base, res, 1.0 + 0.02 * k, 3.0 * k - 9.0) for k in range(9)])
    frames[4, :7, :] = 255
    est = ScaleRotationEstimator(res, M)
    t = torch.from_numpy(frames).to(dev)
    for interp in (INTER_CUBIC, INTER_LANCZOS4):
        got = est.logpolar_batch_device(t, interp).cpu().numpy()
        for k in range(9):
            want = O.logpolar(frames[k], M, interp)
            assert np.array_equal(got[k], want), (res, interp, k, int((got[k] != want).sum()))
            checked += 1
print("remap ok", checked)
# the same forms on full-range, saturating and impulse images (tests/hard_content.py): both clamps, every tap a byte of its own
import hard_content as H
hard = 0
for res, M in ((480, 49.9), (256, 45.0)):
    names, frames = H.remap_batch(500 + res, res, 2 * len(H.REMAP_CLASSES))
    est = ScaleRotationEstimator(res, M)
    t = torch.from_numpy(frames).to(dev)
    for interp in (INTER_CUBIC, INTER_LANCZOS4):
        dst = torch.full(tuple(t.shape), 37, dtype=torch.uint8, device=dev)
        got = est.logpolar_batch_device(t, interp, dst=dst).cpu().numpy()
        for k in range(len(frames)):
            want = O.logpolar(frames[k], M, interp, dst=np.full((res, res), 37, np.uint8))
            if not np.array_equal(got[k], want):
                phi, rho = (int(v) for v in np.argwhere(got[k] != want)[0])
                raise AssertionError((res, interp, names[k], int((got[k] != want).sum()), "first (phi, rho, got, want)", phi, rho,
                                      int(got[k, phi, rho]), int(want[phi, rho])))
            hard += 1
print("hard remap ok", hard)
"""


@pytest.mark.parametrize("env", [{"MOF_SR_LP_RING": "16"}, {"MOF_SR_LP_SUPER": "0"}, {"MOF_SR_LP_STAGED": "0"}, {"MOF_SR_LP_GLOBAL": "1"}])
def test_remap_other_kernel_forms_are_byte_exact(gpu, env):
    """K4's 16-deep ring (maps whose largest super-tile box exceeds 3072 dwords), its one-box-per-wave form (resolutions that
    are not a multiple of 16, boxes beyond 4096 dwords), the table-in-LDS kernel (unaligned layouts) and the per-pixel kernel on
    batches (MOF_SR_LP_GLOBAL=1), forced by their knobs on maps that would take the 12-deep super-tile form: every byte against
    the oracle, on the smooth scenes and on a batch of hard_content's classes (a second count line)."""
    script = _REMAP_SCRIPT.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0 and "remap ok 36" in r.stdout, (env, r.stdout[-1500:], r.stderr[-1500:])
    assert "hard remap ok 104" in r.stdout, (env, r.stdout[-1500:], r.stderr[-1500:])

