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


def _hold(got, b, what, want=None):
    """both slots of every patch of the batch against the f64 oracle at 360 d (`want`: the batch's oracle values gathered for frames
    tiled from its patches)"""
    want = b.want if want is None else want
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), (what, np.argwhere(~np.isfinite(got)).tolist())
    err = np.abs(got - want).reshape(-1, 2).max(axis=0)
    print(f"{what}: max |response - f64 oracle| = {err[0]:.3e}, max |peak - f64 oracle| = {err[1]:.3e}, bar 360 x {b.d:.2e} = {b.bar:.3e} "
          f"({got.shape[0] * got.shape[1]} patches)")
    assert err.max() <= b.bar, (what, err.tolist(), b.bar, np.argwhere(np.abs(got - want) > b.bar).tolist())


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


def _cdc_bar(variant):
    """The bar of a constant pair's peak against the closed form, relative. K1, the half-tile and the planned kernel form C_dc in their own
    tails from the DC bin of the in-LDS transform, the two pixel sums as exact integers: 2^-18.
    The large pipeline (pc_large_kernel.hip) forms it from DC bins of f32 row spectra that went through device memory, and its f32
    roundings are counted instead. On the tuned transforms pcl_cdc_kernel sums line u = 0 in f64 and then: the two sums cast to f32
    (2), their product p4 (1), p4 p4 (1), + 16 eps (1), the hardware reciprocal (1 ulp = 2 half-ulps), the final product (1; the
    factor 4 is exact): 8 half-ulps, each moving the result by at most its own relative size (p4 enters the numerator once and the
    denominator squared: -1 in all). Twice that many: 16 x 2^-24 = 2^-20.
    On L5 - L8 (MOF_FFT_LARGE_TUNED=0, MOF_FFT_FORCE_LARGE, the sizes below 200) the two sums are L6's own bin (0, 0): DC bins of f32
    butterflies, which add integers under unit twiddles and are exact while every partial sum stays below 2^24 -- the doubled pixel
    sum of an image, which _constant_pairs asserts for its frames. The two casts' roundings then stand for nothing larger, the rest
    of the path is the same cross_power_ab, and the count of 8 holds there too."""
    return 16 * 2.0 ** -24 if variant == "planned-large" else 2.0 ** -18


def _constant_pairs(n):
    """texture, a constant frame (81) and an all-zero frame, either way round -- as four pairs and as the five-frame video
    (texture, const, texture, zero, texture) whose pairs they are too; P = the product of the two pixel sums of a constant pair"""
    tex = np.random.default_rng(11).integers(0, 256, (n, n), dtype=np.uint8)
    const, zero = np.full((n, n), 81, np.uint8), np.zeros((n, n), np.uint8)
    P = float(const.astype(np.float64).sum()) * float(tex.astype(np.float64).sum())
    assert 2 * max(int(const.sum(dtype=np.int64)), int(tex.sum(dtype=np.int64))) < 2 ** 24  # (_cdc_bar: exact f32 DC bins)
    return np.stack([const, tex, zero, tex]), np.stack([tex, const, tex, zero]), np.stack([tex, const, tex, zero, tex]), P


def _check_constant_answers(q, n, P, bar, what):
    """q [4, 2]: pairs 0, 1 constant against texture, pairs 2, 3 zero against texture"""
    want_peak = P / (P * P + float(np.finfo(np.float32).eps)) / float(n * n)
    for k in (0, 1):
        rel = abs(q[k, 1] - want_peak) / want_peak
        print(f"{what} constant pair {k}: peak {q[k, 1]:.9e}, closed form {want_peak:.9e}, relative error {rel:.2e} (bar {bar:.2e})")
        assert q[k, 0] == 9.0 * q[k, 1] and q[k, 1] > 0.0, (what, k, q[k])
        assert rel <= bar, (what, k, q[k, 1], want_peak, rel, bar)
    assert (q[2:] == 0.0).all() and not np.signbit(q[2:]).any(), (what, q[2:])


@pytest.mark.parametrize("n", [32, 64, 120, 54, 60, 144, 200, 250])
def test_constant_and_zero_patches(gpu, n):
    """A constant frame (81) and an all-zero frame against texture, either way round: the flat surface C_dc of pc_common.hpp --
    response == 9 peak exactly, peak = C_dc / M^2 with C_dc = P / (P^2 + FLT_EPSILON), P the product of the two pixel sums, at 2^-18
    relative (a handful of f32 roundings and one hardware reciprocal, with 32 ulp of room) where the kernel forms the sums as exact
    integers in its own tail -- K1 (32, 64), the half tile (120, 60 by default, 144), the planned kernel (54) --, at the counted bar of
    _cdc_bar on the large pipeline (200, 250: the tuned transforms, the odd last radix); the zero frame gives exactly (+0, +0). Each
    family decides `degenerate` and forms C_dc in its own code; the variant that ran is printed.
    Under the OpenCL model a constant patch has no finite surface: (NaN, NaN) -- 64, 60 and 144 among these sizes."""
    cur, prev, _, P = _constant_pairs(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1))
    c, p = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    shifts, quality = fm.process_batch_device(c, p, return_quality=True)
    assert _same_bits(shifts, fm.process_batch_device(c, p))
    _check_constant_answers(quality.cpu().numpy()[:, 0], n, P, _cdc_bar(fm.kernel_variant), f"n={n} {fm.kernel_variant}")
    fo = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1), peak_model=PEAK_OCL)
    so, qo = fo.process_batch_device(c, p, return_quality=True)
    print(f"n={n} OpenCL model ({fo.kernel_variant}): (NaN, NaN) on all four pairs")
    assert torch.isnan(qo).all() and torch.isnan(so).all()


@pytest.mark.parametrize("n", [64, 120])
def test_constant_and_zero_frames_in_a_video(gpu, n):
    """The same four pairs as the five-frame video (texture, const, texture, zero, texture): the sequence kernels (pc_seq_kernel.hip at
    64, the half tile's sequence form at 120) pass the constant flags of a frame from `cur` to `prev` of the next pair -- the answers and
    the bars of test_constant_and_zero_patches"""
    _, _, frames, P = _constant_pairs(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1))
    f = torch.from_numpy(frames).to(gpu)
    shifts, quality = fm.process_sequence_device(f, return_quality=True)
    assert _same_bits(shifts, fm.process_sequence_device(f))
    _check_constant_answers(quality.cpu().numpy()[:, 0], n, P, _cdc_bar(fm.kernel_variant), f"n={n} video ({fm.kernel_variant})")


@pytest.mark.parametrize("n,variant", Q.PADDED_SIZES)
def test_zero_and_constant_patches_padded(gpu, n, variant):
    """Padded sizes (62 -> 64, 142 -> 144, 196 -> 200): only the all-zero patch is degenerate there and gives exactly (+0, +0). A constant
    non-zero patch is a box whose answer the oracles do not pin (tests/tolerances.py), so it is held to no value: its quality is finite
    and its shift has the bits of the call without the quality output."""
    cur, prev, _, _ = _constant_pairs(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1))
    assert fm.kernel_variant == variant, fm.kernel_variant
    c, p = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    shifts, quality = fm.process_batch_device(c, p, return_quality=True)
    q = quality.cpu().numpy()[:, 0]
    print(f"n={n} {variant} (M = {O.optimal_dft_size(n)}): constant box {q[0].tolist()} / {q[1].tolist()}, zero patch {q[2].tolist()} / {q[3].tolist()}")
    assert (q[2:] == 0.0).all() and not np.signbit(q[2:]).any(), q[2:]
    assert np.isfinite(q[:2]).all(), q[:2]
    assert _same_bits(shifts, fm.process_batch_device(c, p))


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


# ---- every route the offsets of the quality output take: grids, persistent loops, runs, passes, chunks, the long-range mode, the gate ----
def _batch_engine(b):
    return _engine(b, peak_model=PEAK_OCL) if b.ocl else _engine(b)


def test_grid_order_3x2(gpu):
    """A NON-square grid (3 x 2 patches of 64, 7 pairs) through process_batch_device, process_batch_host and processImage
    (last_quality): a transposed or mis-strided patch index in the quality output is invisible on 2 x 2 only by luck"""
    b = Q.grid64()
    fm = _engine(b)
    assert fm.kernel_variant == "stockham", fm.kernel_variant
    shifts, quality, plain = _pair_entry(fm, b, gpu)
    _hold(quality, b, "n=64 3 x 2 patches, pair entry")
    assert _same_bits(shifts, plain)
    hs, hq = fm.process_batch_host(b.cur, b.prev, return_quality=True)
    _hold(hq, b, "n=64 3 x 2 patches, host entry")
    assert _same_bits(hs, shifts) and _same_bits(hq, quality) and _same_bits(fm.process_batch_host(b.cur, b.prev), shifts)
    ss, sq = [], []
    for k in range(len(b.cur)):
        fm.processImage(b.prev[k])
        ss.append(fm.processImage(b.cur[k]))
        sq.append(fm.last_quality)
    _hold(np.stack(sq), b, "n=64 3 x 2 patches, processImage")
    assert _same_bits(np.stack(ss), shifts) and _same_bits(np.stack(sq), quality)


def _tiled128(pairs=2):
    """The frames of test_gpu_peak_tail.py::test_persistent_form_n128 -- two pairs of a 16 x 16 grid tiled from the 36 circular-shift
    pairs of Q.circular(128), 512 patches against 256 resident workgroups -- and the oracle's quality gathered from those 36
    (`pairs` = 3: 768 patch pairs, more than the 512 slabs of the pair kernel on the half tile at two workgroups per CU)"""
    b, n, g = Q.circular(128), 128, 16
    cur, prev, want = [], [], []
    for k in range(pairs):
        order = [(t + 17 * k) % 36 for t in range(g * g)]
        fc = np.empty((g * n, g * n), np.uint8)
        for t, s in enumerate(order):
            j, i = divmod(t, g)
            fc[j * n:(j + 1) * n, i * n:(i + 1) * n] = b.cur[s]
        cur.append(fc)
        prev.append(np.tile(b.prev[0], (g, g)))
        want.append(b.want[np.asarray(order), 0])
    return b, np.stack(cur), np.stack(prev), np.stack(want)


def _run_tiled128(gpu, variant, pairs=2):
    b, cur, prev, want = _tiled128(pairs)
    fm = FftMethod(sample_point_size=128, max_px_speed=Q.SPEED, frame_shape=cur.shape[1:], grid=(16, 16))
    print(f"route tiled-128{'x3' if pairs == 3 else ''}: kernel_variant {fm.kernel_variant}")
    assert fm.kernel_variant == variant, fm.kernel_variant
    c, p = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    shifts, quality = fm.process_batch_device(c, p, return_quality=True)
    _hold(quality, b, f"n=128 {fm.kernel_variant}, {pairs} x 256 patches tiled from the circular pairs", want=want)
    assert _same_bits(shifts, fm.process_batch_device(c, p))


def test_persistent_form_n128(gpu):
    """K1 at 128 runs a persistent loop: with more patches than resident workgroups every workgroup stores several patches' quality --
    and the pair entry at 128 is held to the oracle at all"""
    _run_tiled128(gpu, "stockham")


def _env_cases(var, default):
    """The (batch name, expectation) cases of a route test: the default route's, or -- in a child process of
    test_gpu_fft_quality_forms.py, where a knob has changed the route -- those of MOF_QUALITY_<var>: 'name=expectation,...'"""
    import os
    v = os.environ.get("MOF_QUALITY_" + var)
    return default if v is None else [tuple(item.split("=")) for item in v.split(",") if item]


_PAIR_ROUTES = [("circular-250", "planned-large"), ("padded-246", "planned-large"), ("crops-400", "planned-large"),
                ("passes-200", "planned-large"), ("ocl-passes-144", "planned-large")]
_LONG_RANGE_ROUTES = [(f"long-range-{n}", v) for n, v in Q.LONG_RANGE_SIZES]
_VIDEO_ROUTES = [("long-video-64", "own"), ("long-video-120", "pair"), ("long-video-128", "own"), ("long-video-200", "pair")]


@pytest.mark.parametrize("name,variant", _env_cases("PAIRS", _PAIR_ROUTES))
def test_pair_entry_on_its_route(gpu, name, variant):
    """A registered batch through the pair entry of the route this process takes, the expected kernel_variant from the parametrisation.
    By default the large pipeline's tuned transforms with an odd last radix (circular 250: 11 gated pairs; 246 padded to 250), 400, and
    the two batches that take several passes of the scratch when MOF_FFT_LARGE_PASS says so (10 pairs at 200, 7 under the OpenCL model
    at 144); test_gpu_fft_quality_forms.py runs it on the knob-selected forms ('tiled-128': the frames of test_persistent_form_n128; 'tiled-128x3': three such pairs)."""
    if name in ("tiled-128", "tiled-128x3"):
        return _run_tiled128(gpu, variant, 3 if name.endswith("x3") else 2)
    b = Q.BATCHES[name]()
    fm = _batch_engine(b)
    print(f"route {name}: kernel_variant {fm.kernel_variant}")
    assert fm.kernel_variant == variant, (name, fm.kernel_variant)
    shifts, quality, plain = _pair_entry(fm, b, gpu)
    if name.startswith("circular-"):
        assert int(torch.isnan(shifts[:, 0, 0]).sum()) == 11 and int(np.isnan(b.shifts[:, 0, 0]).sum()) == 11
    _hold(quality, b, f"{b.name} {fm.kernel_variant}, pair entry")
    assert _same_bits(shifts, plain)


@pytest.mark.parametrize("name,variant", _env_cases("LONG_RANGE", _LONG_RANGE_ROUTES))
def test_long_range_beyond_32(gpu, name, variant):
    """The long-range mode (4n x 4n frames, sqNum = 4: one quarter-resolution patch of n pixels) beyond K1 at 32: the planned kernel
    (60), the tuned 120 kernel's DS = 4 front end (pc_kernel_mixed.hip), the large pipeline's L5 - L8 (200) -- long-range launches stay
    on the family's kernel, kernel_variant names the full-resolution route. At 120 also the stateful processImageLongRange."""
    b = Q.BATCHES[name]()
    fm = FftMethod(4 * b.n, b.n, Q.SPEED)
    print(f"route {name}: kernel_variant {fm.kernel_variant}")
    assert fm.kernel_variant == variant, (name, fm.kernel_variant)
    c, p = torch.from_numpy(b.cur).to(gpu), torch.from_numpy(b.prev).to(gpu)
    shifts, quality = fm.process_long_range_batch_device(c, p, return_quality=True)
    _hold(quality, b, f"{b.name}, batch entry")
    assert _same_bits(shifts, fm.process_long_range_batch_device(c, p))
    if b.n == 120:
        for k in (1, 3):
            fm.processImageLongRange(b.prev[k])
            s = fm.processImageLongRange(b.cur[k])
            assert _same_bits(s, shifts[k]) and _same_bits(fm.last_quality, quality[k])


@pytest.mark.parametrize("name,bits", _env_cases("VIDEOS", _VIDEO_ROUTES))
def test_sequence_runs(gpu, name, bits):
    """process_sequence_device on videos longer than one run of the sequence kernels: 37 pairs of 3 patches at 64 (runs of 2 with
    nothing forced), 21 and 10 pairs on the half tile's sequence form at 120 and 128 (runs of 4, a ragged last one), 10 pairs of the
    large video form at 200 -- every run but the first stores its quality at a non-zero pair offset. bits = 'pair': the video entry
    has the pair entry's bits, shifts and quality (120 and 200 by default, test_video_entries; every size under MOF_FFT_SEQ_PAIRS);
    'own': it has NOT -- 64 and 128 by default, where the video runs a kernel of its own that transforms every frame alone while the
    pair kernel packs cur + i prev into one complex transform: other roundings, so equal bits on every patch of these videos would
    mean that the pair form ran (what a child of test_gpu_fft_quality_forms.py that selects the pair form is told apart by)."""
    b = Q.BATCHES[name]()
    fm = _engine(b)
    frames = torch.from_numpy(b.frames).to(gpu)
    shifts, quality = fm.process_sequence_device(frames, return_quality=True)
    _hold(quality, b, f"{b.name} video entry ({fm.kernel_variant})")
    assert _same_bits(shifts, fm.process_sequence_device(frames))
    ps, pq = fm.process_batch_device(frames[1:], frames[:-1], return_quality=True)
    _hold(pq, b, f"{b.name} pair entry ({fm.kernel_variant})")
    same = _same_bits(shifts, ps) and _same_bits(quality, pq)
    print(f"route {name}: kernel_variant {fm.kernel_variant}, video entry == pair entry bits: {same}")
    assert bits in ("pair", "own") and same == (bits == "pair"), (name, bits, same)


def test_host_entry_chunks(gpu):
    """process_batch_host(..., return_quality=True) on the 7 pairs of 3 x 2 patches, and on 7 pairs as a video (cur = frames[1:],
    prev = frames[:-1] of ONE array of eight frames: the pipeline uploads every frame once): the device entry's bits, shifts and
    quality, through the HostPipe with two outputs -- in one chunk by default, either form in four chunks with a ragged last one
    under MOF_HOST_CHUNK=2"""
    b = Q.grid64()
    fm = _engine(b)
    shifts, quality, _ = _pair_entry(fm, b, gpu)
    _hold(quality, b, "n=64 3 x 2 patches, pair entry")
    hs, hq = fm.process_batch_host(b.cur, b.prev, return_quality=True)
    assert _same_bits(hs, shifts) and _same_bits(hq, quality)
    frames = np.concatenate([b.cur, b.prev[:1]])  # (any eight frames, seven pairs: bits against bits)
    f = torch.from_numpy(frames).to(gpu)
    vs, vq = fm.process_batch_device(f[1:], f[:-1], return_quality=True)
    hs, hq = fm.process_batch_host(frames[1:], frames[:-1], return_quality=True)
    assert hs.shape == (7, 6, 2) and np.isfinite(hq).all()
    assert _same_bits(hs, vs) and _same_bits(hq, vq)


def _gate_split(b):
    """A small max_px_speed for the batch, chosen from the f64 oracle's shifts alone: the middle of the widest gap between two
    consecutive magnitudes that leaves at least a quarter of the patches on either side; (value, [pairs, patches] gated)"""
    mag = np.hypot(b.shifts[..., 0], b.shifts[..., 1])
    m = np.sort(mag[np.isfinite(mag)])
    quarter = -(-mag.size // 4)
    best = None
    for i in range(quarter, len(m) - quarter + 1):  # m[:i] pass, m[i:] are gated
        if best is None or m[i] - m[i - 1] > best[0]:
            best = (m[i] - m[i - 1], 0.5 * (m[i] + m[i - 1]))
    assert best is not None, b.name
    return best[1], mag > best[1]


@pytest.mark.parametrize("name", ["crops-64", "circular-120", "circular-54", "circular-200"])
def test_quality_does_not_depend_on_the_speed_gate(gpu, name):
    """include/mof.h: the quality does not depend on the gate -- here the max_px_speed gate (the +-n/2 gate: test_parity_per_family).
    Two engines, max_px_speed = Q.SPEED and a small value: the same quality bits; the shifts NaN exactly where the f64 oracle's shift
    exceeds the small value (or leaves +-n/2), the same bits elsewhere. K1 (crops-64), the half tile (120), the planned kernel (54),
    the large pipeline (200); the circular pairs' shifts are known integers."""
    b = Q.BATCHES[name]()
    small, gated = _gate_split(b)
    mag = np.hypot(b.shifts[..., 0], b.shifts[..., 1])
    finite = np.isfinite(mag)
    margin = float(np.abs(mag[finite] - small).min())
    print(f"{b.name}: max_px_speed {small:.4f} px gates {int(gated.sum())} and passes {int((finite & ~gated).sum())} of {mag.size} patches "
          f"({int((~finite).sum())} beyond +-n/2), nearest oracle magnitude {margin:.3f} px away")
    assert 4 * int(gated.sum()) >= mag.size and 4 * int((finite & ~gated).sum()) >= mag.size and margin > 1e-3
    h, w = b.cur.shape[1:3]
    wide = _engine(b)
    tight = FftMethod(sample_point_size=b.n, max_px_speed=small, frame_shape=(h, w), grid=b.grid)
    c, p = torch.from_numpy(b.cur).to(gpu), torch.from_numpy(b.prev).to(gpu)
    ws, wq = wide.process_batch_device(c, p, return_quality=True)
    ts, tq = tight.process_batch_device(c, p, return_quality=True)
    _hold(tq, b, f"{b.name} ({tight.kernel_variant}) under max_px_speed = {small:.3f}")
    assert _same_bits(tq, wq), "the quality must not depend on the gate"
    assert _same_bits(ts, tight.process_batch_device(c, p))
    ws, ts = ws.cpu().numpy(), ts.cpu().numpy()
    want_nan = gated | ~finite
    assert np.array_equal(np.isnan(ts[..., 0]), want_nan) and np.array_equal(np.isnan(ts[..., 1]), want_nan), np.argwhere(np.isnan(ts[..., 0]) != want_nan).tolist()
    assert _same_bits(ts[~want_nan], ws[~want_nan])


@pytest.mark.parametrize("n,variant", Q.SPLIT_SIZES)
def test_launch_split_after_65535_pairs(gpu, n, variant):
    """The pair kernels carry the pair index in gridDim.z, so a batch goes out in launches of 65535 frame pairs and the second
    launch's quality pointer is offset on its own line (pc_kernel.hip, pc_kernel_generic.hip, pc_half_kernel.hip): 65 540 pairs of
    one small patch, of period 8 -- pair k must carry the bits of pair k mod 8 (same patches, same kernel) and the first eight the
    f64 oracle's values at 360 d. (The sequence entry's split: test_gpu_fft_sequence.py. The large pipeline splits only inside a
    pass of 65535 PATCH pairs of at least 136 pixels, which is no test input: launch_pcl_peak's offset is not reached.)"""
    b = Q.split_period(n)
    fm = FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1))
    assert fm.kernel_variant == variant, fm.kernel_variant
    protos = torch.from_numpy(b.protos.copy()).to(gpu)
    k = torch.arange(65535 + 5, device=gpu) % 8
    cur, prev = protos[(k + 1) % 8], protos[k]
    shifts, quality = fm.process_batch_device(cur, prev, return_quality=True)
    assert _same_bits(shifts, fm.process_batch_device(cur, prev))
    _hold(quality[:8], b, f"n={n} {variant}, first period of {len(k)} pairs")
    q = _bits(quality)
    off = np.argwhere((q != q[:8][k.cpu().numpy()]).any(axis=(1, 2))).ravel()
    print(f"n={n} {variant}: {len(k) - off.size} of {len(k)} pairs carry the bits of their pair of the first period")
    assert off.size == 0, (off[:4].tolist(), int(off.size))
