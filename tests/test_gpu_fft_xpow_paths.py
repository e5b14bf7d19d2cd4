"""Which form of the normalised cross-power spectrum a bin takes -- C = P' rsq(q) where q = |P'|^2 >= 1024, the general form below
(csrc/pc_common.hpp) -- is decided per bin INSIDE a batch of a lane's bins: one test and one branch per batch, the general form behind
it. The rest of the suite meets the main form everywhere and the all-general case only through constant patches, whose answer is the
degenerate substitute: the general form's result is never looked at there. The fixtures tests/golden/xpow_paths_*.npz (made by
tests/golden/make_xpow_paths.py, which describes them) mix the two forms inside one lane's batch, across the lanes of a wave and across
the waves of a workgroup, on ONE 64 x 64 or 32 x 32 patch per pair; every pair goes through the pair entry and the video entry and is
held to both oracles under tolerances.check_patch_strict with no relaxation: nothing may be recorded."""
import os

import numpy as np
import pytest
import torch

import tolerances
from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _q(cur, prev):
    """q of every bin in float64; the four real-only slots (another form) at +inf"""
    a, b = np.fft.fft2(cur.astype(np.float64)), np.fft.fft2(prev.astype(np.float64))
    q = 16.0 * np.abs(a) ** 2 * np.abs(b) ** 2
    h = cur.shape[0] // 2
    q[np.ix_((0, h), (0, h))] = np.inf
    return q


def _run(name, n, gpu):
    g = np.load(os.path.join(GOLDEN, f"xpow_paths_{name}_n{n}.npz"))
    cur, prev = g["cur"], g["prev"]
    fm = FftMethod(sample_point_size=n, frame_shape=(n, n), grid=(1, 1))
    tc, tp = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    out = {"pair": fm.process_batch_device(tc, tp).cpu().numpy()[:, 0],
           "video": np.stack([fm.process_sequence_device(torch.stack([tp[k], tc[k]])).cpu().numpy()[0, 0] for k in range(len(cur))])}
    first = len(tolerances.RECORDS)
    for entry, got in out.items():
        for k in range(len(cur)):
            w64, w32 = g["oracle64"][k, 0], g["oracle32"][k, 0]
            print(f"xpow paths {name} n={n} {entry} pair {k}: got {got[k].tolist()} f64 oracle {w64.tolist()} |got - f64| {np.abs(got[k] - w64).max():.3g} "
                  f"|got - f32| {np.abs(got[k] - w32).max():.3g} |f32 - f64| {np.abs(w32 - w64).max():.3g}")
    for entry, got in out.items():
        for k in range(len(cur)):
            tolerances.check_patch_strict(got[k], g["oracle64"][k, 0], g["oracle32"][k, 0], f"xpow paths/{name}_n{n}/{entry}", k)
    assert len(tolerances.RECORDS) == first, tolerances.RECORDS[first:]  # the plain bar: no relaxation used
    return g, [_q(cur[k], prev[k]) for k in range(len(cur))]


@pytest.mark.parametrize("n", [64, 32])
def test_one_large_bin_among_a_lanes_small_ones(gpu, n):
    """The period-4 pattern (three large bins, the others exactly zero) and one raised pixel (magnitude 2 in every bin): the lane that owns
    column n/4 of row n/4 holds one bin of the main form and seven of the general one. The oracles return the planted shift to 2e-14 px."""
    g, qs = _run("mixed", n, gpu)
    for k, q in enumerate(qs):
        assert q[n // 4, n // 4] >= 1024.0 and q[3 * n // 4, 3 * n // 4] >= 1024.0
        small = q < 1024.0
        assert small.sum() == n * n - 6 and np.allclose(q[small], 256.0)  # (3 pattern bins, 3 more real-only slots)
        assert np.abs(g["oracle64"][k, 0] - g["shifts"][k]).max() < 1e-12


@pytest.mark.parametrize("n", [64, 32])
def test_lanes_of_both_forms_in_every_wave(gpu, n):
    """An 8 x 8 integer tile repeated over the patch: the bins on the multiples of n/8 are large, every other bin holds the raised pixel
    alone -- whole lanes on the main form beside whole lanes on the general one."""
    _, qs = _run("tile", n, gpu)
    for q in qs:
        on = np.zeros(q.shape, bool)
        on[::n // 8, ::n // 8] = True
        assert (q[~on] < 1024.0).all() and (q[on] >= 1024.0).sum() >= 40 and (q[on] < 1024.0).sum() <= 24


@pytest.mark.parametrize("n", [64, 32])
def test_one_wave_takes_the_branch(gpu, n):
    """The pattern, the raised pixel and a weak texture: a handful of bins below the threshold, all in the spectrum rows of one wave of the
    inverse row pass (n = 64: pair k -> wave k, rows 8k .. 8k + 7 and their Hermitian partners; n = 32 has one wave)."""
    _, qs = _run("one_wave", n, gpu)
    for k, q in enumerate(qs):
        rows = np.unique(np.nonzero(q < 1024.0)[0])
        assert 0 < (q < 1024.0).sum() <= 8 and (q >= 1024.0).sum() >= n * n - 12
        if n == 64:
            assert {min(v, n - v) // 8 for v in rows} == {k} and 0 not in rows and n // 2 not in rows


@pytest.mark.parametrize("n", [64, 32])
def test_branch_not_taken(gpu, n):
    """Textured pairs whose smallest q is far above the threshold."""
    _, qs = _run("main", n, gpu)
    assert min(q.min() for q in qs) >= 1024.0
