"""GPU tests of the per-patch correlation quality (response, peak) of every FFT entry (include/mof.h, "Per-patch correlation quality").

Reference: the f64 CPU oracle's diagnostics (oracle_pc_diag.response, .peak_value), on batches whose every pair has one clear peak
(test_fft_quality_host.py proves that for each of them on the CPU). Bar: 360 d, d the distance between the f32 and the f64 oracle on
the SAME batch (tests/quality_cases.py) -- the ratio the project's shift bar (1e-4 px) has over the oracles' mutual distance on the
circular-shift pairs (2.8e-7 px): the kernels differ from the f32 oracle by transform order and 1-ulp rsq / rcp, which the shift bar
already grants. Nothing here is tuned from what the kernels return; each test prints what it measured (run with -s)."""
import numpy as np
import pytest
import torch

import oracle_lib as O
import quality_cases as Q
from mrs_optic_flow_amd import FftMethod
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _engine(b, **kw):
    h, w = b.cur.shape[1:3]
    return FftMethod(sample_point_size=b.n, max_px_speed=Q.SPEED, frame_shape=(h, w), grid=b.grid, **kw)


def _hold(got, b, what):
    """both slots of every patch of the batch against the f64 oracle at 360 d"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == b.want.shape and got.dtype == np.float64, (what, got.shape, b.want.shape)
    assert np.isfinite(got).all(), (what, np.argwhere(~np.isfinite(got)).tolist())
    err = np.abs(got - b.want).reshape(-1, 2).max(axis=0)
    print(f"{what}: max |response - f64 oracle| = {err[0]:.3e}, max |peak - f64 oracle| = {err[1]:.3e}, bar 360 x {b.d:.2e} = {b.bar:.3e} "
          f"({got.shape[0] * got.shape[1]} patches)")
    assert err.max() <= b.bar, (what, err.tolist(), b.bar, np.argwhere(np.abs(got - b.want) > b.bar).tolist())


def _pair_entry(fm, b, gpu):
    """(shifts, quality) of the pair entry and, separately, its shifts without the quality output"""
    c, p = torch.from_numpy(b.cur).to(gpu), torch.from_numpy(b.prev).to(gpu)
    shifts, quality = fm.process_batch_device(c, p, return_quality=True)
    plain = fm.process_batch_device(c, p)
    torch.cuda.synchronize()
    return shifts, quality, plain


@pytest.mark.parametrize("n,variant", Q.CIRCULAR_SIZES)
def test_parity_per_family(gpu, n, variant):
    """The 36 circular-shift pairs of test_gpu_peak_tail.py (peak on every corner and edge; 11 gated): K1 (32, 64), the half-tile kernel
    (120), the planned kernel (54), the large-patch pipeline (200). The gated pairs' shift is NaN, their quality finite and held."""
    b = Q.circular(n)
    fm = _engine(b)
    assert fm.kernel_variant == variant, fm.kernel_variant
    shifts, quality, plain = _pair_entry(fm, b, gpu)
    assert int(torch.isnan(shifts[:, 0, 0]).sum()) == 11 and int(np.isnan(b.shifts[:, 0, 0]).sum()) == 11
    _hold(quality, b, f"n={n} {variant}")
    assert _same_bits(shifts, plain), "the shifts must not depend on the quality output"


@pytest.mark.parametrize("n,variant", Q.PADDED_SIZES)
def test_padded_sizes(gpu, n, variant):
    """Patches that cv::phaseCorrelate pads: 62 (M = 64, planned), 142 (M = 144, half tile), 196 (M = 200, large); quality is per M^2"""
    b = Q.padded(n)
    fm = _engine(b)
    assert fm.kernel_variant == variant, fm.kernel_variant
    shifts, quality, plain = _pair_entry(fm, b, gpu)
    _hold(quality, b, f"n={n} {variant} (M = {O.optimal_dft_size(n)})")
    assert _same_bits(shifts, plain)


@pytest.mark.parametrize("n", Q.VIDEO_SIZES)
def test_video_entries(gpu, n):
    """process_sequence_device on a 5-frame video of two patches per frame: the sequence kernels of 64, 120, 128 and the large video form"""
    b = Q.video(n)
    fm = _engine(b)
    frames = torch.from_numpy(b.frames).to(gpu)
    shifts, quality = fm.process_sequence_device(frames, return_quality=True)
    plain = fm.process_sequence_device(frames)
    _hold(quality, b, f"n={n} video ({fm.kernel_variant})")
    assert _same_bits(shifts, plain)
    if n in (120, 200):  # the video form has the pair entry's bits at these sizes (test_gpu_fft_sequence.py): so has its quality
        ps, pq = fm.process_batch_device(frames[1:], frames[:-1], return_quality=True)
        assert _same_bits(shifts, ps) and _same_bits(quality, pq)


def test_bgr8_n64(gpu):
    """BGR8 frames: the quality bits of the gray entry on the gray conversion of the same frames (pair and video entries)"""
    b = Q.crops64()
    rng = np.random.default_rng(3)
    tint = rng.integers(0, 40, (2,) + b.cur.shape + (3,))
    bgr_c = np.clip(b.cur[..., None].astype(np.int64) + tint[0], 0, 255).astype(np.uint8)
    bgr_p = np.clip(b.prev[..., None].astype(np.int64) + tint[1], 0, 255).astype(np.uint8)
    gray_c, gray_p = np.stack([O.rgb2gray(f) for f in bgr_c]), np.stack([O.rgb2gray(f) for f in bgr_p])
    fm = _engine(b)
    s3, q3 = fm.process_batch_device_bgr(torch.from_numpy(bgr_c).to(gpu), torch.from_numpy(bgr_p).to(gpu), return_quality=True)
    s1, q1 = fm.process_batch_device(torch.from_numpy(gray_c).to(gpu), torch.from_numpy(gray_p).to(gpu), return_quality=True)
    assert _same_bits(s3, s1) and _same_bits(q3, q1) and np.isfinite(q1.cpu().numpy()).all()
    v3, vq3 = fm.process_sequence_device_bgr(torch.from_numpy(bgr_c).to(gpu), return_quality=True)
    v1, vq1 = fm.process_sequence_device(torch.from_numpy(gray_c).to(gpu), return_quality=True)
    assert _same_bits(v3, v1) and _same_bits(vq3, vq1)


def test_long_range(gpu):
    """128 x 128 frames, patch size 32 (sqNum = 4: one quarter-resolution patch) against the oracle on the oracle's quarter resize"""
    b = Q.long_range()
    fm = FftMethod(128, 32, Q.SPEED)
    c, p = torch.from_numpy(b.cur).to(gpu), torch.from_numpy(b.prev).to(gpu)
    shifts, quality = fm.process_long_range_batch_device(c, p, return_quality=True)
    _hold(quality, b, "long range 128 / 32")
    assert _same_bits(shifts, fm.process_long_range_batch_device(c, p))
    fm.processImageLongRange(b.prev[0])
    s = fm.processImageLongRange(b.cur[0])
    assert _same_bits(s, shifts[0]) and _same_bits(fm.last_quality, quality[0])


def test_stateful_and_host_entries_n64(gpu):
    """processImage twice -> last_quality; process_batch_host on 5 pairs: the device batch entry's bits on the same frames"""
    b = Q.crops64()
    fm = _engine(b)
    shifts, quality, _ = _pair_entry(fm, b, gpu)
    _hold(quality, b, "n=64 pair entry, 2 x 2 patches")
    hs, hq = fm.process_batch_host(b.cur, b.prev, return_quality=True)
    assert hq.shape == (5, 4, 2) and _same_bits(hs, shifts) and _same_bits(hq, quality)
    assert _same_bits(fm.process_batch_host(b.cur, b.prev), shifts)
    fm.processImage(b.prev[2])
    s = fm.processImage(b.cur[2])
    assert fm.last_quality.shape == (4, 2) and _same_bits(s, shifts[2]) and _same_bits(fm.last_quality, quality[2])


@pytest.mark.parametrize("n", [32, 64])
def test_constant_and_zero_patches(gpu, n):
    """A constant frame (81) and an all-zero frame against texture, either way round: the flat surface C_dc of pc_common.hpp --
    response == 9 peak exactly, peak = C_dc / M^2 with C_dc = P / (P^2 + FLT_EPSILON), P the product of the two pixel sums, at 2^-18
    relative (a handful of f32 roundings and one hardware reciprocal, with 32 ulp of room); the zero frame gives exactly (0, 0).
    Under the OpenCL model a constant patch has no finite surface: (NaN, NaN)."""
    tex = np.random.default_rng(11).integers(0, 256, (n, n), dtype=np.uint8)
    const, zero = np.full((n, n), 81, np.uint8), np.zeros((n, n), np.uint8)
    cur = np.stack([const, tex, zero, tex])
    prev = np.stack([tex, const, tex, zero])
    fm = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1))
    c, p = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    q = fm.process_batch_device(c, p, return_quality=True)[1].cpu().numpy()[:, 0]
    P = float(const.astype(np.float64).sum()) * float(tex.astype(np.float64).sum())
    want_peak = P / (P * P + float(np.finfo(np.float32).eps)) / float(n * n)
    for k in (0, 1):
        rel = abs(q[k, 1] - want_peak) / want_peak
        print(f"n={n} constant pair {k}: peak {q[k, 1]:.9e}, closed form {want_peak:.9e}, relative error {rel:.2e} (bar 2^-18 = {2.0 ** -18:.2e})")
        assert q[k, 0] == 9.0 * q[k, 1] and q[k, 1] > 0.0, (k, q[k])
        assert rel <= 2.0 ** -18, (k, q[k, 1], want_peak, rel)
    assert (q[2:] == 0.0).all() and not np.signbit(q[2:]).any(), q[2:]
    fo = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1), peak_model=PEAK_OCL)
    so, qo = fo.process_batch_device(c, p, return_quality=True)
    assert torch.isnan(qo).all() and torch.isnan(so).all()


def test_discrimination_n64(gpu):
    """A loose sanity check of what the number is for: an identical pair answers > 0.9, independent noise < 0.25 (oracle: 0.99, <= 0.14)"""
    rng = np.random.default_rng(5)
    a, b2 = rng.integers(0, 256, (2, 64, 64), dtype=np.uint8)
    fm = FftMethod(sample_point_size=64, max_px_speed=Q.SPEED, frame_shape=(64, 64), grid=(1, 1))
    cur, prev = torch.from_numpy(np.stack([a, a])).to(gpu), torch.from_numpy(np.stack([a, b2])).to(gpu)
    q = fm.process_batch_device(cur, prev, return_quality=True)[1].cpu().numpy()[:, 0, 0]
    print(f"n=64 response: identical pair {q[0]:.4f}, independent noise {q[1]:.4f}")
    assert q[0] > 0.9 and q[1] < 0.25, q


@pytest.mark.parametrize("n,variant", Q.OCL_SIZES)
def test_opencl_model(gpu, n, variant):
    """MOF_PEAK_OCL: refine()'s 7 x 7 positive-only sum and the first maximum of the scaled surface, against fft_process_ocl's diagnostics;
    the bar from that model's two oracles"""
    b = Q.ocl(n)
    fm = _engine(b, peak_model=PEAK_OCL)
    assert fm.kernel_variant == variant, fm.kernel_variant
    shifts, quality, plain = _pair_entry(fm, b, gpu)
    _hold(quality, b, f"OpenCL model n={n} {variant}")
    assert _same_bits(shifts, plain)


def test_graph_replay_n64(gpu):
    """One process_batch_device(..., return_quality=True) captured on a side stream after an eager warm-up (a single-branch graph),
    replayed once: the eager call's bits"""
    from mrs_optic_flow_amd import release_captured

    b = Q.crops64()
    fm = _engine(b)
    c, p = torch.from_numpy(b.cur).to(gpu), torch.from_numpy(b.prev).to(gpu)
    ws, wq = fm.process_batch_device(c, p, return_quality=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gs, gq = fm.process_batch_device(c, p, return_quality=True)
    gs.zero_()
    gq.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert _same_bits(gs, ws) and _same_bits(gq, wq)
    del g
    release_captured(fm)
