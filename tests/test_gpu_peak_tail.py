"""GPU tests of the peak tails (arg-max butterfly, 5 x 5 window, fp64 centroid butterfly, gate) of every kernel family that takes the
cross-lane helpers of csrc/pc_common.hpp (lane_xor / wave_best / wave_sum3), with the peak ON EVERY CORNER AND EDGE of the shifted
surface: one random n x n patch, the current image its circular shift by (dy, dx), dy, dx in {0, +-1, +-(n/2 - 1), -n/2} -- 36
pairs per size in one batch. The window is then clamped on one or two sides (zero lanes in the centroid sum) or lies in the
interior; shifts with a -n/2 component put the centroid beyond the +-n/2 gate and must come out NaN. `max_px_speed` is large, so
no other gate acts. Bar: the f64 oracle at 1e-4 px, the same NaN pattern, no patch relaxed or left out (on these pairs the f32 and
f64 oracles agree within 2.8e-7 px and on the NaN pattern at every size used here -- checked once on the CPU)."""
import functools

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import FftMethod
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu
TOL = 1e-4
SPEED = 1.0e4  # px: only the +-n/2 gate acts


def _shifts(n):
    vals = (0, 1, -1, n // 2 - 1, -(n // 2 - 1), -(n // 2))
    return [(dy, dx) for dy in vals for dx in vals]


@functools.lru_cache(maxsize=None)
def _case(n):
    """prev [n, n], cur [36, n, n] and the f64 oracle's [36, 2] -- computed once per size, shared, read-only"""
    prev = np.random.default_rng(7).integers(0, 256, (n, n), dtype=np.uint8)
    cur = np.stack([np.roll(prev, s, axis=(0, 1)) for s in _shifts(n)])
    lay = O.fft_layout(n, n, n, 1, 1, max_px_speed=SPEED)
    want = np.stack([O.fft_process(c, prev, lay, 64)[0][0] for c in cur])
    for a in (prev, cur, want):
        a.setflags(write=False)
    return prev, cur, want


def _check(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, np.argwhere(np.isnan(got) != np.isnan(want)).tolist())
    err = np.nan_to_num(np.abs(got - want))
    print(f"{what}: max |got - f64 oracle| = {err.max():.3e} px, {int(np.isnan(want[..., 0]).sum())} of {want.shape[0]} gated")
    assert err.max() <= TOL, (what, float(err.max()), np.argwhere(err > TOL).tolist())


@pytest.mark.parametrize("n,variant", [(32, "stockham"), (64, "stockham"), (120, "planned-half"), (54, "planned"), (200, "planned-large")])
def test_peak_on_every_corner_and_edge(gpu, n, variant):
    """One patch per frame, 36 pairs in one batch: K1 (32, 64), K1h (120), the planned kernel (54), the large-patch pipeline (200)."""
    prev, cur, want = _case(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=SPEED, frame_shape=(n, n), grid=(1, 1))
    assert fm.kernel_variant == variant, fm.kernel_variant
    assert int(np.isnan(want[:, 0]).sum()) == 11 and not np.isnan(want[0]).any()  # the pairs with a -n/2 component are gated, no other
    c = torch.from_numpy(np.ascontiguousarray(cur)).to(gpu)
    p = torch.from_numpy(np.ascontiguousarray(prev)).to(gpu).expand(len(cur), n, n).contiguous()
    got = fm.process_batch_device(c, p).cpu().numpy()[:, 0]
    _check(got, want, f"n={n} {fm.kernel_variant}")
    if n == 120:  # the video form has the pair entry's bits at this size (test_gpu_fft_sequence.py asserts it): still so, pair by pair
        for k in (0, 7, 35):
            seq = fm.process_sequence_device(torch.stack([p[k], c[k]])).cpu().numpy()[0, 0]
            assert np.array_equal(seq, got[k], equal_nan=True), (k, seq, got[k])


@functools.lru_cache(maxsize=None)
def _case_ocl(n):
    """the same 36 pairs under the OpenCL kernel's peak model with search_radius = n (no row or column masked): the f64 oracle's [36, 2]"""
    prev, cur, _ = _case(n)
    lay = O.fft_layout(n, n, n, 1, 1, max_px_speed=SPEED)
    want = np.stack([O.fft_process_ocl(c, prev, lay, search_radius=n, precision=64)[0][0] for c in cur])
    want.setflags(write=False)
    return want


@pytest.mark.parametrize("n,variant", [(64, "stockham"), (60, "planned"), (144, "planned-large")])
def test_ocl_window_clamped_at_every_corner_and_edge(gpu, n, variant):
    """The OpenCL model's 7 x 7 window (49 lanes, values > 0 only) clamped at the surface's edges: K1 (64), the planned kernel (60), the
    large-patch pipeline (144). With only positive values in a window clamped at 0 the centroid cannot leave +-n/2: no pair is gated
    (on these pairs the f32 and f64 oracles agree within 3.7e-6 / 4.4e-6 / 1.35e-5 px and on the NaN pattern -- checked once on the CPU)."""
    prev, cur, _ = _case(n)
    want = _case_ocl(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=SPEED, frame_shape=(n, n), grid=(1, 1), peak_model=PEAK_OCL, search_radius=n)
    assert fm.kernel_variant == variant, fm.kernel_variant
    assert not np.isnan(want).any()
    c = torch.from_numpy(np.ascontiguousarray(cur)).to(gpu)
    p = torch.from_numpy(np.ascontiguousarray(prev)).to(gpu).expand(len(cur), n, n).contiguous()
    got = fm.process_batch_device(c, p).cpu().numpy()[:, 0]
    _check(got, want, f"n={n} {fm.kernel_variant} OpenCL model")


def _tiled(n, g, order):
    """frames of g x g patches: prev everywhere the same patch, cur patch t its shift number order[t]"""
    prev, cur, want = _case(n)
    fp = np.tile(prev, (g, g))
    fc = np.empty_like(fp)
    for t, s in enumerate(order):
        j, i = divmod(t, g)
        fc[j * n:(j + 1) * n, i * n:(i + 1) * n] = cur[s]
    return fp, fc, want[np.asarray(order)]


def test_sequence_entry_n64(gpu):
    """K1's sequence kernel (pc_seq_kernel.hip): a 2-frame video whose frame holds a 6 x 6 grid of 64 x 64 patches, one shift each."""
    n, g = 64, 6
    fp, fc, want = _tiled(n, g, list(range(36)))
    fm = FftMethod(sample_point_size=n, max_px_speed=SPEED, frame_shape=(g * n, g * n), grid=(g, g))
    got = fm.process_sequence_device(torch.from_numpy(np.stack([fp, fc])).to(gpu)).cpu().numpy()
    assert got.shape == (1, 36, 2)
    _check(got[0], want, "n=64 sequence")


def test_persistent_form_n128(gpu):
    """N = 128, 2 pairs of a 16 x 16 grid: 512 patches against 256 resident workgroups, so the persistent form's tail runs with the
    next patch behind it (its second barrier holds the other waves off the tile until the window is read)."""
    n, g = 128, 16
    want_all = []
    cur, prev = [], []
    for k in range(2):
        fp, fc, want = _tiled(n, g, [(t + 17 * k) % 36 for t in range(g * g)])
        prev.append(fp)
        cur.append(fc)
        want_all.append(want)
    fm = FftMethod(sample_point_size=n, max_px_speed=SPEED, frame_shape=(g * n, g * n), grid=(g, g))
    got = fm.process_batch_device(torch.from_numpy(np.stack(cur)).to(gpu), torch.from_numpy(np.stack(prev)).to(gpu)).cpu().numpy()
    _check(got.reshape(-1, 2), np.concatenate(want_all), f"n=128 {fm.kernel_variant}")
