"""GPU tests of the log-polar remap (csrc/sr_kernel.hip, launch_sr_logpolar and its kernel forms) on the images of tests/hard_content.py:
full-range, saturating and impulse content, every byte against the oracle. The smooth scenes of sr_scenes.py never drive a footprint's sum
below zero and move a destination byte by a fraction of an LSB when a tap is misplaced; here both clamps run on thousands of pixels per
frame (asserted) and an impulse turns every tap's position and weight into a destination byte of its own. The estimator's three entries are
then held to one another, by equality only, on a video of the same classes."""
import numpy as np
import pytest
import torch

import hard_content as H
import oracle_lib as O
from mrs_optic_flow_amd import ScaleRotationEstimator
from mrs_optic_flow_amd.engine import INTER_CUBIC, INTER_LANCZOS4

pytestmark = pytest.mark.gpu
FILL = 37  # former content of the destination: BORDER_TRANSPARENT pixels must keep it


def assert_remap_equal(got, want, names, what):
    """got, want: [n, res, res] uint8. On a difference: how many bytes differ, and the first one as (image class, phi, rho, got, want)."""
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    k, phi, rho = (int(v) for v in bad[0])
    per_image = {names[i]: int((got[i] != want[i]).sum()) for i in sorted({int(b[0]) for b in bad})}
    raise AssertionError(f"{what}: {len(bad)} bytes differ; first: class {names[k]} (image {k}), phi {phi}, rho {rho}, got {int(got[k, phi, rho])}, "
                         f"want {int(want[k, phi, rho])}; per image: {per_image}")


def clamp_counts(frame, M, interp, variant):
    """Valid pixels of one frame whose real-valued interpolation sum lies below -0.5 / above 255.5 (the float64 gather of hard_content):
    the pixels on which the lower / upper clamp decides the byte."""
    mx, my = O.logpolar_maps(frame.shape[0], M, variant)
    ref, valid = H.logpolar_gather_f64(frame, mx, my, interp)
    return int((valid & (ref < -0.5)).sum()), int((valid & (ref > 255.5)).sum())


# (240, 40), (256, 45), (480, 49.9): the 12-deep super-tile form; (480, 30): boxes beyond the staged kernel's reach, the table-in-LDS kernel;
# (480, 80): the small boxes, every ring class; 200: not a multiple of 16, the one-box-per-wave staged form
@pytest.mark.parametrize("res,M", [(240, 40.0), (256, 45.0), (480, 49.9), (480, 30.0), (480, 80.0), (200, 35.0)])
@pytest.mark.parametrize("interp", [INTER_CUBIC, INTER_LANCZOS4])
@pytest.mark.parametrize("variant", [0, 1])
def test_logpolar_remap_is_byte_exact_on_hard_content(gpu, res, M, interp, variant):
    """Every class of hard_content.REMAP_CLASSES in one batch (dark and bright frames next to each other in the staged kernel's ring), through
    the per-pixel kernel (n = 1), the staged kernel with full and ragged ring groups (n = 5, 37), from a pitched view, onto a non-zero
    destination, and from a layout of odd pitch and frame stride (staged from unaligned dwords, the last image per pixel)."""
    n_max = 37
    names, frames = H.remap_batch(7 * res + interp, res, n_max)
    assert set(H.REMAP_CLASSES) <= set(names)
    # a condition, not a measurement: the batch really clamps, on both sides (one binary-noise frame alone is enough)
    below, above = clamp_counts(frames[names.index("binary_noise")], M, interp, variant)
    assert below >= 1000 and above >= 1000, (below, above)
    est = ScaleRotationEstimator(res, M, logpolar_variant=variant)
    want = np.stack([O.logpolar(f, M, interp, dst=np.full((res, res), FILL, np.uint8), variant=variant) for f in frames])
    assert int((want == FILL).sum()) > n_max * res  # the outermost rings map outside the source: transparent pixels are in play
    big = torch.zeros((n_max, res + 2, res + 24), dtype=torch.uint8, device=gpu)
    big[:, 1:1 + res, 8:8 + res] = torch.from_numpy(frames).to(gpu)
    view = big[:, 1:1 + res, 8:8 + res]  # pitch > res, crop origin passed as the pointer
    for n_img in (1, 5, n_max):
        dst = torch.full((n_img, res, res), FILL, dtype=torch.uint8, device=gpu)
        got = est.logpolar_batch_device(view[:n_img], interp, dst=dst).cpu().numpy()
        assert_remap_equal(got, want[:n_img], names, f"res {res} M {M} interp {interp} variant {variant}, batch of {n_img}")
    # the per-pixel kernel on more than the first class: a binary-noise, a holes, a checker and a split frame alone
    for k in (names.index("binary_noise"), names.index("holes"), names.index("checker1"), names.index("halves_h")):
        dst = torch.full((1, res, res), FILL, dtype=torch.uint8, device=gpu)
        got = est.logpolar_batch_device(view[k:k + 1], interp, dst=dst).cpu().numpy()
        assert_remap_equal(got, want[k:k + 1], names[k:k + 1], f"res {res} M {M} interp {interp} variant {variant}, single image")
    # odd pitch and frame stride: the staged kernel reads unaligned dwords for n - 1 images, the per-pixel kernel takes the last
    lo, n_odd = 1, 8
    odd = torch.zeros((n_odd, res + 1, res + 7), dtype=torch.uint8, device=gpu)
    assert odd.stride(0) % 4 != 0 or odd.stride(1) % 4 != 0
    odd[:, 1:1 + res, 3:3 + res] = torch.from_numpy(frames[lo:lo + n_odd]).to(gpu)
    dst = torch.full((n_odd, res, res), FILL, dtype=torch.uint8, device=gpu)
    got = est.logpolar_batch_device(odd[:, 1:1 + res, 3:3 + res], interp, dst=dst).cpu().numpy()
    assert_remap_equal(got, want[lo:lo + n_odd], names[lo:lo + n_odd], f"res {res} M {M} interp {interp} variant {variant}, odd pitch")
    # default destination = zeros (tempIm, scaleRotationEstimator.cpp:27): transparent pixels read 0
    zero = est.logpolar_batch_device(view[:6], interp).cpu().numpy()
    want0 = np.stack([O.logpolar(f, M, interp, variant=variant) for f in frames[:6]])
    assert_remap_equal(zero, want0, names[:6], f"res {res} M {M} interp {interp} variant {variant}, zero destination")


@pytest.mark.parametrize("res,M,chunk", [(240, 40.0, 5), (480, 49.9, 0), (200, 35.0, 4)])
def test_estimator_entries_agree_bit_for_bit_on_hard_content(gpu, res, M, chunk):
    """A video of the hard classes through the three entries of the estimator: the sequence entry returns what the stateful call returns frame by
    frame, and a pair of the batch entry returns what a fresh estimator returns for (prev, cur) -- stateful or as a two-frame sequence --
    [scale, rot, pt] bit for bit (the same kernels run). Equality only: binary noise through a log-polar map is outside what f32 transforms
    pin against the oracle, and that belongs to tests/tolerances.py, not here."""
    n = len(H.REMAP_CLASSES) + 2
    names, frames = H.remap_batch(3 * res + 1, res, n)
    wide = torch.zeros((n, res + 2, res + 24), dtype=torch.uint8, device=gpu)
    wide[:, 1:1 + res, 8:8 + res] = torch.from_numpy(frames).to(gpu)
    video = wide[:, 1:1 + res, 8:8 + res]
    seq_engine = ScaleRotationEstimator(res, M, batch_chunk=chunk)
    seq = seq_engine.process_sequence_device(video).cpu().numpy()
    assert np.isfinite(seq).all() and tuple(seq[0]) == (1.0, 0.0, 0.0, 0.0)
    one = ScaleRotationEstimator(res, M)
    for k in range(n):
        s, r = one.processImage(frames[k])
        assert (s, r) == (seq[k, 0], seq[k, 1]), (k, names[k], s, r, seq[k])
    batch = ScaleRotationEstimator(res, M, batch_chunk=chunk).process_batch_device(video[1:], video[:-1]).cpu().numpy()
    assert np.array_equal(batch[0], seq[1]), (batch[0], seq[1])  # the first pair of a fresh sequence IS a fresh estimator's pair
    for k in range(n - 1):
        fresh = ScaleRotationEstimator(res, M)
        assert fresh.processImage(frames[k]) == (1.0, 0.0)
        s, r = fresh.processImage(frames[k + 1])
        assert (s, r) == (batch[k, 0], batch[k, 1]), (k, names[k], names[k + 1], s, r, batch[k])
        two = ScaleRotationEstimator(res, M).process_sequence_device(video[k:k + 2]).cpu().numpy()
        assert np.array_equal(two[1], batch[k]), (k, names[k], names[k + 1], two[1], batch[k])
        alone = ScaleRotationEstimator(res, M).process_batch_device(video[k + 1:k + 2], video[k:k + 1]).cpu().numpy()
        assert np.array_equal(alone[0], batch[k]), (k, alone[0], batch[k])
