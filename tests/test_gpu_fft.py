"""GPU parity tests of K1 (FFT phase correlation) through the C ABI, against the CPU oracle.

Tolerance: 1e-4 px (BASELINE.json north_star) on well-conditioned patches -- a clear single
peak, second-highest surface value outside the 5x5 window below half the peak. On the rest
(flat / ambiguous patches, where the arg-max itself is decided by rounding noise) the GPU must
agree with the oracle on validity (NaN or not) unless the oracle's own f32/f64 variants disagree.
"""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import FftMethod, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TOL = 1e-4


def _compare(got, cur, prev, lay, label=""):
    want64, _, diags = O.fft_process(cur, prev, lay, 64, want_diag=True)
    want32, _ = O.fft_process(cur, prev, lay, 32)
    well = np.array([d.second_value < 0.5 * d.peak_value for d in diags])
    n_checked = 0
    for p in range(want64.shape[0]):
        if well[p]:
            assert np.allclose(got[p], want64[p], rtol=0, atol=TOL, equal_nan=True), (label, p, got[p], want64[p])
            assert np.allclose(got[p], want32[p], rtol=0, atol=TOL, equal_nan=True), (label, p, got[p], want32[p])
            n_checked += 1
        elif np.array_equal(np.isnan(want64[p]), np.isnan(want32[p])) and np.allclose(want64[p], want32[p], rtol=0, atol=TOL, equal_nan=True):
            # the two oracle precisions agree, so the surface has a stable arg-max: so must the GPU
            assert np.allclose(got[p], want64[p], rtol=0, atol=TOL, equal_nan=True), (label, "ill", p, got[p], want64[p])
    return n_checked


@pytest.mark.parametrize("name", ["fft_n64_unaligned.npz", "fft_n128.npz", "fft_n32_tiled.npz",
                                  "fft_n120_reference_tiling.npz"])
def test_golden_vectors(gpu, name):
    g = np.load(os.path.join(GOLDEN, name))
    w, h, n, gx, gy, ox, oy, sx, sy = (int(v) for v in g["layout"])
    fm = FftMethod(sample_point_size=n, frame_shape=(h, w), grid=(gx, gy), origin=(ox, oy), stride=(sx, sy))
    got = fm.process_batch_device(torch.from_numpy(g["cur"]).to(gpu), torch.from_numpy(g["prev"]).to(gpu)).cpu().numpy()
    ok = g["well_conditioned"]
    assert ok.sum() > 0.8 * ok.size
    assert np.allclose(got[ok], g["expected"][ok], rtol=0, atol=TOL, equal_nan=True)
    # validity must agree wherever the arg-max is not decided by rounding noise (a constant patch at N = 120 has
    # AC bins of pure rounding noise under radix-3/5 butterflies, in the oracle as on the GPU)
    stable = ok | (g["kinds"][:, None] != "constant")
    assert np.array_equal(np.isnan(got)[stable], np.isnan(g["expected"])[stable])
    # the host-pointer batch entry gives the same bits as the device-pointer one
    got_h = fm.process_batch_host(g["cur"], g["prev"])
    assert np.array_equal(got_h, got, equal_nan=True)


@pytest.mark.parametrize("n,shape,grid,origin,stride", [
    (64, (480, 752), (8, 8), (1, 1), (98, 59)),        # BASELINE c2 layout
    (128, (270, 480), (3, 2), (0, 0), (119, 63)),      # c4 patch/stride on a reduced frame
    (64, (448, 448), (7, 7), (0, 0), (64, 64)),        # the reference's own square tiling (sqNum = 7)
    (32, (70, 130), (3, 1), (2, 3), (33, 1)),
    (120, (480, 480), (4, 4), (0, 0), (120, 120)),     # the reference's default geometry (default.yaml:31-32)
    (120, (250, 380), (3, 2), (3, 1), (127, 129)),
])
def test_seeded_batches_match_oracle(gpu, n, shape, grid, origin, stride):
    h, w = shape
    B = 6
    cur, prev, shifts, kinds = synth.batch_np(B, h, w, n // 8, k0=0)
    fm = FftMethod(sample_point_size=n, frame_shape=shape, grid=grid, origin=origin, stride=stride)
    got = fm.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)).cpu().numpy()
    lay = O.fft_layout(w, h, n, grid[0], grid[1], origin, stride)
    checked = sum(_compare(got[k], cur[k], prev[k], lay, f"pair{k}/{kinds[k]}") for k in range(B))
    assert checked > 0.7 * B * grid[0] * grid[1]
    for k in range(B):
        if kinds[k] == "shift":
            assert np.allclose(np.nanmedian(got[k], axis=0), shifts[k], rtol=0, atol=0.5)


def test_pitch_and_frame_stride_are_honoured(gpu):
    """Frames embedded in a larger allocation: row pitch > width, pair stride > frame, video-style cur/prev."""
    h, w, n = 96, 160, 64
    frames = np.stack([synth.pair_np(9, h, w, 2 * t, -t)[0] for t in range(4)])  # a 4-frame sequence
    big = torch.zeros((4, h + 5, w + 24), dtype=torch.uint8, device=gpu)
    big[:, 2:2 + h, 8:8 + w] = torch.from_numpy(frames).to(gpu)
    view = big[:, 2:2 + h, 8:8 + w]
    fm = FftMethod(sample_point_size=n, frame_shape=(h, w), grid=(2, 1), origin=(5, 7), stride=(90, 1))
    got = fm.process_batch_device(view[1:], view[:-1]).cpu().numpy()  # cur = frames[1:], prev = frames[:-1]
    lay = O.fft_layout(w, h, n, 2, 1, (5, 7), (90, 1))
    for t in range(3):
        want, _ = O.fft_process(frames[t + 1], frames[t], lay, 64)
        assert np.allclose(got[t], want, rtol=0, atol=TOL, equal_nan=True)


def test_stateful_processimage_mirrors_the_reference(gpu):
    """first frame correlates with itself (FftMethod.cpp:1791-1793), then prev <- cur (:1872); setImPrev does not
    clear `first`; reset() re-arms it."""
    fs, n = 128, 64
    seq = [synth.pair_np(21, fs, fs, 3 * t, 2 * t, blur=True)[0] for t in range(3)]
    fm = FftMethod(fs, n, 80.0)
    assert (fm.cfg.grid_x, fm.cfg.grid_y) == (2, 2) and fm.sqNum == 2
    lay = O.fft_layout(fs, fs, n, 2, 2)
    fm.setImPrev(np.zeros((fs, fs), np.uint8))  # what the nodelet does at start-up (optic_flow.cpp:1016-1018)
    out0 = fm.processImage(seq[0])
    assert np.allclose(out0, O.fft_process(seq[0], seq[0], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    assert np.allclose(out0, 0.0, rtol=0, atol=1e-5)
    out1 = fm.processImage(seq[1])
    assert np.allclose(out1, O.fft_process(seq[1], seq[0], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    out2 = fm.processImage(np.ascontiguousarray(seq[2]))
    assert np.allclose(out2, O.fft_process(seq[2], seq[1], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    fm.reset()
    assert np.allclose(fm.processImage(seq[0]), out0, rtol=0, atol=0, equal_nan=True)
    # a strided (non-contiguous rows) cv::Mat-like view is accepted through `pitch`
    wide = np.zeros((fs, fs + 40), np.uint8)
    wide[:, 10:10 + fs] = seq[1]
    out1b = fm.processImage(wide[:, 10:10 + fs])
    assert np.allclose(out1b, out1, rtol=0, atol=0, equal_nan=True)


def test_gating_constant_and_large_shift(gpu):
    n = 64
    const = np.full((n, n), 200, np.uint8)
    fm = FftMethod(n, n, 80.0)
    out = fm.process_batch_host(const[None], const[None])[0]
    assert np.allclose(out, O.fft_process(const, const, O.fft_layout(n, n, n, 1, 1), 32)[0], rtol=0, atol=1e-6)
    assert np.allclose(out, 1 - n / 2, rtol=0, atol=1e-4)  # same degenerate answer as the CPU path (see test_oracle_fft)
    fm_small = FftMethod(n, n, 9.99)
    prev = synth.canvas_np(3, n, n, False)[:n, :n].copy()
    cur = np.roll(prev, (0, 10), axis=(0, 1))
    assert np.isnan(fm_small.process_batch_host(cur[None], prev[None])).all()
    assert np.allclose(FftMethod(n, n, 10.01).process_batch_host(cur[None], prev[None])[0], [[10.0, 0.0]], rtol=0, atol=1e-5)
    fm128 = FftMethod(128, 128, 80.0)
    c128 = np.full((128, 128), 9, np.uint8)
    assert np.isnan(fm128.process_batch_host(c128[None], c128[None])).all()  # (-63,-63) exceeds 80 px


@pytest.mark.parametrize("n", [32, 64, 128, 120])
def test_one_constant_patch_gives_the_reference_degenerate_answer(gpu, n):
    """cv::phaseCorrelate transforms the two patches separately: a CONSTANT patch has an exactly zero AC spectrum, the
    surface is flat and the answer is the first-index / 3 x 3-centroid artefact 9c / (9c + DBL_EPSILON) - N/2 (or -N/2 for
    an all-zero patch) -- deterministic, and what the gate then sees. The packed two-for-one transform of K1 leaked rounding
    noise into those zeros and answered with noise (found by tools/fft_sr_fuzz.py in round 3); constant patches are now
    detected at the load. Checked against the oracle patch by patch (N = 120: the oracle's own radix-3/5 DFT of a constant
    is not exactly zero, so there the closed form is the reference)."""
    tex = synth.canvas_np(5, n, n, True)[:n, :n].copy()
    tex2 = synth.canvas_np(6, n, n, True)[:n, :n].copy()
    c77, zero = np.full((n, n), 77, np.uint8), np.zeros((n, n), np.uint8)
    pairs = [(tex, c77), (c77, tex), (tex, zero), (zero, tex), (c77, c77), (zero, zero), (c77, zero), (tex, tex2)]
    cur = np.stack([a for a, _ in pairs])
    prev = np.stack([b for _, b in pairs])
    fm = FftMethod(n, n, 1000.0)  # gate wide open: the values themselves are compared
    got = fm.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)).cpu().numpy()[:, 0]
    lay = O.fft_layout(n, n, n, 1, 1)
    lay.max_px_speed = 1000.0
    for k, (a, b) in enumerate(pairs[:-1]):
        if n == 120:
            sa, sb = float(a.astype(np.float64).sum()), float(b.astype(np.float64).sum())
            pdc = sa * sb
            c = pdc / (pdc * pdc + np.finfo(np.float32).eps) if pdc > 0 else 0.0
            want = (9 * c / (9 * c + np.finfo(np.float64).eps) if c > 0 else 0.0) - n / 2
            assert np.allclose(got[k], want, rtol=0, atol=1e-4), (n, k, got[k], want)
        else:
            want = O.fft_process(a, b, lay, 32)[0][0]
            assert np.allclose(got[k], want, rtol=0, atol=TOL), (n, k, got[k], want)
            assert np.allclose(want, O.fft_process(a, b, lay, 64)[0][0], rtol=0, atol=1e-9)
    assert np.isfinite(got[-1]).all()  # an ordinary pair in the same batch is untouched
    # through the gate of a real configuration (max_px_speed 80): (1 - N/2, 1 - N/2) is valid at N = 64, invalid at N = 128 / 120
    gated = FftMethod(n, n, 80.0).process_batch_device(torch.from_numpy(cur[:2]).to(gpu), torch.from_numpy(prev[:2]).to(gpu)).cpu().numpy()[:, 0]
    assert np.isnan(gated).all() == (2 * (n / 2 - 1) ** 2 > 80.0 ** 2)
    if n == 120:  # long-range mode: constancy is judged on the quarter-resolution pixels the kernel forms on the fly
        lr = FftMethod(480, 120, 1000.0)
        big = synth.canvas_np(12, 480, 480, True)[:480, :480].copy()
        lr.processImageLongRange(big)
        res = lr.processImageLongRange(np.full((480, 480), 50, np.uint8))[0]
        q = O.resize_quarter(big).astype(np.float64)
        pdc = q.sum() * 50.0 * 120 * 120
        c = pdc / (pdc * pdc + np.finfo(np.float32).eps)
        assert np.allclose(res, 9 * c / (9 * c + np.finfo(np.float64).eps) - 60, rtol=0, atol=1e-4), res
    # a frame with a constant rectangle: only the patches inside it are degenerate, in the stateful entry as well
    if n == 64:
        frame_a = synth.canvas_np(9, 192, 192, True)[:192, :192].copy()
        frame_b = synth.canvas_np(10, 192, 192, True)[:192, :192].copy()
        frame_b[:64, 64:128] = 200
        f3 = FftMethod(192, 64, 1000.0)
        lay3 = O.fft_layout(192, 192, 64, 3, 3)
        lay3.max_px_speed = 1000.0
        f3.processImage(frame_a)
        res = f3.processImage(frame_b)
        want = O.fft_process(frame_b, frame_a, lay3, 32)[0]
        assert np.allclose(res[1], want[1], rtol=0, atol=TOL) and abs(res[1][0] + 31) < 1e-3


def test_circular_shifts_are_exact(gpu):
    n = 64
    prev = synth.canvas_np(11, n, n, False)[:n, :n].copy()
    shifts = [(5, -3), (-7, 2), (0, 11), (-1, -1), (13, 13), (-20, 6)]
    cur = np.stack([np.roll(prev, (dy, dx), axis=(0, 1)) for dx, dy in shifts])
    fm = FftMethod(n, n, 80.0)
    got = fm.process_batch_host(cur, np.repeat(prev[None], len(shifts), 0))[:, 0]
    assert np.allclose(got, np.array(shifts, float), rtol=0, atol=2e-5)


def test_full_size_c2_batch_properties(gpu):
    """BASELINE config c2 at full size (752x480, 8x8 x 64^2, batch 1024): size-independent properties
    instead of 65k oracle calls -- planted translation recovered per pair, identical frames give ~0,
    the batch result equals the per-pair result bit for bit, and a sample is checked against the oracle."""
    B, h, w, n = 1024, 480, 752, 64
    cur, prev, shifts, kinds = synth.batch_torch(B, h, w, n // 8, gpu)
    fm = FftMethod(sample_point_size=n, frame_shape=(h, w), grid=(8, 8), origin=(1, 1), stride=(98, 59))
    out = fm.process_batch_device(cur, prev)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    sh = shifts.numpy()
    for k in range(B):
        if kinds[k] in ("shift", "noisy"):
            assert np.isfinite(res[k]).all()
            assert np.abs(np.median(res[k], axis=0) - sh[k]).max() < 0.3, (k, kinds[k])
            assert np.abs(res[k] - sh[k]).max() < 1.0
        elif kinds[k] == "identical":
            assert np.abs(res[k]).max() < 1e-4
        else:
            assert np.allclose(res[k], 1 - n / 2, rtol=0, atol=1e-4)
    # independence: pair k alone gives the same bits
    for k in (0, 511, 1023):
        alone = fm.process_batch_device(cur[k:k + 1], prev[k:k + 1]).cpu().numpy()[0]
        assert np.array_equal(alone, res[k], equal_nan=True)
    lay = O.fft_layout(w, h, n, 8, 8, (1, 1), (98, 59))
    for k in (1, 500, 1011):
        _compare(res[k], cur[k].cpu().numpy(), prev[k].cpu().numpy(), lay, f"full{k}")


@pytest.mark.parametrize("fs,n", [(512, 64), (1024, 128), (256, 32), (960, 120)])
def test_long_range_mode(gpu, fs, n):
    """processImageLongRange: quarter-resolution patches formed inside the kernel; shares `first`/prev with
    processImage (FftMethod.cpp:1920-1922, :1992, :2004). Every patch size has its own load path (sqNum = 8 -> sqNum_lr = 2)."""
    seq = [synth.pair_np(41, fs, fs, 8 * t, -4 * t)[0] for t in range(3)]
    lay = O.fft_layout(fs, fs, n, 8, 8)
    fm = FftMethod(fs, n, 80.0)
    out0 = fm.processImageLongRange(seq[0])
    assert out0.shape == (4, 2)
    assert np.allclose(out0, O.fft_process_long_range(seq[0], seq[0], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    out1 = fm.processImageLongRange(seq[1])
    assert np.allclose(out1, O.fft_process_long_range(seq[1], seq[0], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    if n >= 64:  # (a quarter-resolution 32-px patch of this texture is too coarse for the planted motion; parity above holds)
        assert np.allclose(out1, [2.0, -1.0], rtol=0, atol=0.3)
    out2 = fm.processImage(seq[2])  # the ordinary path continues from the same previous frame
    assert np.allclose(out2, O.fft_process(seq[2], seq[1], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    cur = torch.from_numpy(np.stack(seq[1:])).to(gpu)
    prev = torch.from_numpy(np.stack(seq[:-1])).to(gpu)
    got = fm.process_long_range_batch_device(cur, prev).cpu().numpy()
    for t in range(2):
        want, _ = O.fft_process_long_range(seq[t + 1], seq[t], lay, 64)
        assert np.allclose(got[t], want, rtol=0, atol=TOL, equal_nan=True)
    from mrs_optic_flow_amd import MofError
    with pytest.raises(MofError):  # sqNum < 4
        FftMethod(128, 64, 80.0).processImageLongRange(np.zeros((128, 128), np.uint8))


def test_reference_default_geometry_480_120(gpu):
    """frame_size 480, sample_point_size 120 (config/default.yaml:31-32): the stateful path and long-range mode
    (sqNum 4 -> sqNum_lr 1) on the patch size the reference actually ships with."""
    fs, n = 480, 120
    seq = [synth.pair_np(51, fs, fs, 8 * t, 4 * t)[0] for t in range(3)]
    lay = O.fft_layout(fs, fs, n, 4, 4)
    fm = FftMethod(fs, n, 80.0)
    assert fm.sqNum == 4
    fm.processImage(seq[0])
    out1 = fm.processImage(seq[1])
    assert np.allclose(out1, O.fft_process(seq[1], seq[0], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    assert np.allclose(np.median(out1, axis=0), [8.0, 4.0], rtol=0, atol=0.3)
    out2 = fm.processImageLongRange(seq[2])
    assert out2.shape == (1, 2)
    assert np.allclose(out2, O.fft_process_long_range(seq[2], seq[1], lay, 64)[0], rtol=0, atol=TOL, equal_nan=True)
    # circular shifts on a single 120x120 patch are exact
    prev = synth.canvas_np(12, n, n, False)[:n, :n].copy()
    shifts = [(7, -9), (-30, 11), (1, 0)]
    cur = np.stack([np.roll(prev, (dy, dx), axis=(0, 1)) for dx, dy in shifts])
    got = FftMethod(n, n, 80.0).process_batch_host(cur, np.repeat(prev[None], 3, 0))[:, 0]
    assert np.allclose(got, np.array(shifts, float), rtol=0, atol=3e-5)


@pytest.mark.parametrize("n,fs", [(64, 256), (120, 240), (128, 256), (32, 96)])
def test_bgr_front_end_fused_into_the_load(gpu, n, fs):
    """BGR8 camera frames, crop at (xi, yi) and CV_RGB2GRAY (optic_flow.cpp:1609-1622) fused into K1."""
    B, H, W, xi, yi = 3, fs + 17, fs + 40, 23, 9
    rng = np.random.default_rng(77)
    base = [synth.pair_np(60 + k, H, W, 3 + k, -2 * k) for k in range(B)]
    # colour frames whose gray conversion is non-trivial: channels = texture scaled/offset differently + noise
    def colour(g):
        g = g.astype(np.int32)
        ch = np.stack([g, 255 - g // 2, (g * 3 // 4 + 20)], axis=-1) + rng.integers(-2, 3, g.shape + (3,))
        return np.clip(ch, 0, 255).astype(np.uint8)
    cur = np.stack([colour(c) for c, _ in base])
    prev = np.stack([colour(p) for _, p in base])
    fm = FftMethod(fs, n, 80.0)
    tc, tp = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    got = fm.process_batch_device_bgr(tc[:, yi:yi + fs, xi:xi + fs], tp[:, yi:yi + fs, xi:xi + fs]).cpu().numpy()
    lay = O.fft_layout(fs, fs, n, fs // n, fs // n)
    for k in range(B):
        gc = O.rgb2gray(cur[k, yi:yi + fs, xi:xi + fs])
        gp = O.rgb2gray(prev[k, yi:yi + fs, xi:xi + fs])
        _compare(got[k], gc, gp, lay, f"bgr{k}")
        # identical bits to running the gray path on the converted crop
        ref = fm.process_batch_device(torch.from_numpy(gc[None]).to(gpu), torch.from_numpy(gp[None]).to(gpu)).cpu().numpy()[0]
        assert np.array_equal(ref, got[k], equal_nan=True)


def test_edge_cases_and_error_paths(gpu):
    """Empty batches, shape mismatches, unsupported geometry, engine reuse across many calls."""
    from mrs_optic_flow_amd import MofError, _capi
    import ctypes as C

    fm = FftMethod(128, 64, 80.0)
    empty = torch.zeros((0, 128, 128), dtype=torch.uint8, device=gpu)
    assert fm.process_batch_device(empty, empty).shape == (0, 4, 2)
    assert fm.process_batch_host(np.zeros((0, 128, 128), np.uint8), np.zeros((0, 128, 128), np.uint8)).shape == (0, 4, 2)
    with pytest.raises(ValueError):
        fm.processImage(np.zeros((64, 64), np.uint8))
    with pytest.raises(MofError) as exc:
        FftMethod(sample_point_size=1000, frame_shape=(1000, 1000))  # pads to 1000: beyond the planned transforms (<= 960)
    assert exc.value.code == _capi.MOF_ERR_UNSUPPORTED
    assert FftMethod(sample_point_size=48, frame_shape=(96, 96)).kernel_variant == "planned"  # (any other size has a kernel, r04)
    lib = _capi.load()
    assert lib.mof_fft_process_batch_device(fm._h, None, 0, None, 0, 128, 1, None, None) == _capi.MOF_ERR_BAD_ARG
    assert b"bad batch" in lib.mof_last_error()
    # an engine is reusable: alternate stateful and batched calls, results stay those of a fresh engine
    f = [synth.pair_np(70, 128, 128, 2 * t, t)[0] for t in range(3)]
    fresh = FftMethod(128, 64, 80.0)
    fresh.processImage(f[0]); want = fresh.processImage(f[1])
    for _ in range(3):
        fm.reset(); fm.processImage(f[0])
        fm.process_batch_host(np.stack(f), np.stack(f[::-1]))
        assert np.array_equal(fm.processImage(f[1]), want, equal_nan=True)


def test_batch_entry_points_are_hip_graph_capturable(gpu):
    """No allocation, synchronisation or host read-back inside the batched entry points: they can be captured into a
    HIP graph on the caller's stream and replayed (launch-bound pipelines such as c5 benefit)."""
    from mrs_optic_flow_amd import ScaleRotationEstimator

    B, fs = 4, 256
    cur, prev, _, _ = synth.batch_np(B, fs, fs, 6, classes=False, k0=3)
    tc, tp = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    fm, sr = FftMethod(fs, 64, 80.0), ScaleRotationEstimator(fs, 45.0)
    out = torch.empty((B, fm.n_patches, 2), dtype=torch.float64, device=gpu)
    want = fm.process_batch_device(tc, tp).clone()
    want_sr = sr.process_batch_device(tc, tp).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    # (engines of earlier tests may be finalised by Python's collector INSIDE this capture: the library frees under the
    # relaxed capture mode, so that does not invalidate it -- no gc.disable() here any more)
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            fm.process_batch_device(tc, tp, out=out)
            sr_out = sr.process_batch_device(tc, tp)
    out.zero_()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(sr_out, want_sr)


# ---- the useOCL=true peak model (MOF_PEAK_OCL) ----------------------------------------------
# Tolerances: 1e-4 px against the oracle's double evaluation of the model; 5e-4 px against its faithful float
# evaluation, whose centroid sums floats over ABSOLUTE frame coordinates and so carries up to ~2e-4 px of rounding
# noise of its own (tests/test_oracle_fft.py::test_ocl_model_f32_noise_floor) -- the engine sums patch-local doubles.
TOL_OCL_F32 = 5e-4


def _compare_ocl(got, cur, prev, lay, sr=55, label=""):
    want64, _, diags = O.fft_process_ocl(cur, prev, lay, sr, 64, want_diag=True)
    want32, _ = O.fft_process_ocl(cur, prev, lay, sr, 32)
    n_checked = 0
    for p in range(want64.shape[0]):
        d = diags[p]
        if np.isfinite(d.peak_value) and d.second_value < 0.5 * d.peak_value:
            assert np.allclose(got[p], want64[p], rtol=0, atol=TOL, equal_nan=True), (label, p, got[p], want64[p])
            assert np.allclose(got[p], want32[p], rtol=0, atol=TOL_OCL_F32, equal_nan=True), (label, p, got[p], want32[p])
            n_checked += 1
    return n_checked


@pytest.mark.parametrize("n,shape,grid,origin,stride", [
    (64, (480, 752), (8, 8), (1, 1), (98, 59)),
    (128, (270, 480), (3, 2), (0, 0), (119, 63)),
    (32, (70, 130), (3, 1), (2, 3), (33, 1)),
    (120, (480, 480), (4, 4), (0, 0), (120, 120)),   # the geometry the OpenCL kernel is launched with (SEARCH_RADIUS 55 < 60)
])
def test_ocl_peak_model_matches_oracle(gpu, n, shape, grid, origin, stride):
    from mrs_optic_flow_amd.engine import PEAK_OCL
    h, w = shape
    B = 6
    cur, prev, shifts, kinds = synth.batch_np(B, h, w, n // 8, k0=100)
    fm = FftMethod(sample_point_size=n, frame_shape=shape, grid=grid, origin=origin, stride=stride, peak_model=PEAK_OCL)
    got = fm.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)).cpu().numpy()
    lay = O.fft_layout(w, h, n, grid[0], grid[1], origin, stride)
    checked = sum(_compare_ocl(got[k], cur[k], prev[k], lay, 55, f"pair{k}/{kinds[k]}") for k in range(B))
    assert checked > 0.6 * B * grid[0] * grid[1]
    # the two peak models are different estimators: same motion, different sub-pixel value
    cv = FftMethod(sample_point_size=n, frame_shape=shape, grid=grid, origin=origin, stride=stride)
    got_cv = cv.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)).cpu().numpy()
    for k in range(B):
        if kinds[k] == "shift":
            assert np.allclose(np.nanmedian(got[k], axis=0), shifts[k], rtol=0, atol=0.5)
            assert np.nanmax(np.abs(got[k] - got_cv[k])) > 10 * TOL


def test_ocl_peak_model_mask_constant_and_modes(gpu):
    from mrs_optic_flow_amd.engine import PEAK_OCL
    n = 64
    prev = synth.canvas_np(7, n, n, False)[:n, :n].copy()
    cur = np.roll(prev, (0, 9), axis=(0, 1))
    lay = O.fft_layout(n, n, n, 1, 1)
    wide = FftMethod(n, n, 80.0, peak_model=PEAK_OCL, search_radius=12).process_batch_host(cur[None], prev[None])[0]
    assert np.allclose(wide, [[9.0, 0.0]], rtol=0, atol=2e-5)
    # search radius 5: the true peak is masked. What is left is rounding noise of ~1e-8, far below the FLT_EPSILON the
    # centroid's sum is seeded with, so the estimate collapses towards -N/2 (cl:1342, :1366): anything but (9, 0).
    narrow = FftMethod(n, n, 80.0, peak_model=PEAK_OCL, search_radius=5).process_batch_host(cur[None], prev[None])[0]
    assert np.all(np.isnan(narrow) | (narrow < -n / 4)), narrow
    # constant patches: the real-only slots are 1/0 (cl:1029) -> (NaN, NaN), unlike the cv::phaseCorrelate model
    const = np.full((n, n), 200, np.uint8)
    fm = FftMethod(n, n, 80.0, peak_model=PEAK_OCL)
    assert np.isnan(fm.process_batch_host(const[None], const[None])).all()
    assert np.isnan(O.fft_process_ocl(const, const, lay)[0]).all()
    # stateful + long-range entry points run the same model
    fs = 512
    seq = [synth.pair_np(43, fs, fs, 8 * t, -4 * t)[0] for t in range(3)]
    lay8 = O.fft_layout(fs, fs, n, 8, 8)
    fm = FftMethod(fs, n, 80.0, peak_model=PEAK_OCL)
    fm.processImage(seq[0])
    out1 = fm.processImage(seq[1])
    assert _compare_ocl(out1, seq[1], seq[0], lay8, 55, "stateful") > 40
    out2 = fm.processImageLongRange(seq[2])
    q1, q2 = O.resize_quarter(seq[1]), O.resize_quarter(seq[2])
    assert _compare_ocl(out2, q2, q1, O.fft_layout(fs // 4, fs // 4, n, 2, 2), 55, "long-range") >= 3
    # BGR front end
    col = lambda g: np.stack([g, 255 - g // 2, g // 4 * 3 + 20], axis=-1).astype(np.uint8)
    c3, p3 = col(seq[2]), col(seq[1])
    got = fm.process_batch_device_bgr(torch.from_numpy(c3[None]).to(gpu), torch.from_numpy(p3[None]).to(gpu)).cpu().numpy()[0]
    assert _compare_ocl(got, O.rgb2gray(c3), O.rgb2gray(p3), lay8, 55, "bgr") > 40
    from mrs_optic_flow_amd import MofError
    with pytest.raises(MofError):
        FftMethod(n, n, 80.0, peak_model=7)


def test_expected_variant(gpu):
    assert FftMethod(64, 64, 80.0).kernel_variant == "stockham"
    assert FftMethod(128, 128, 80.0).kernel_variant == "stockham"


def test_more_pairs_than_one_grid_dimension_holds(gpu):
    """64 x 64 patches run one workgroup per patch with the pair index on gridDim.z (at most 65535): a longer batch is
    split into several launches inside the library. Circular shifts are exact, so every pair has a known answer."""
    n, B = 64, 65535 + 9
    gen = torch.Generator(device="cpu").manual_seed(5)
    base = torch.randint(0, 256, (n, n), dtype=torch.uint8, generator=gen)
    shifts = [(3, -2), (-5, 7), (0, 1), (11, 0)]
    protos = torch.stack([torch.roll(base, (dy, dx), dims=(0, 1)) for dx, dy in shifts]).to(gpu)
    idx = torch.arange(B, device=gpu) % len(shifts)
    cur = protos[idx]                                   # [B, 64, 64]
    prev = base.to(gpu).expand(B, n, n)                 # stride-0 batch: every pair shares one previous frame
    fm = FftMethod(n, n, 80.0)
    got = fm.process_batch_device(cur, prev.contiguous()).cpu().numpy()[:, 0]
    want = np.array(shifts, float)[idx.cpu().numpy()]
    assert np.allclose(got, want, rtol=0, atol=3e-5)
    assert np.allclose(got[65533:65540], want[65533:65540], rtol=0, atol=3e-5)  # across the launch boundary
