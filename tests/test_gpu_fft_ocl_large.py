"""GPU tests of the OpenCL kernel's peak model (MOF_PEAK_OCL, useOCL=true) on patches too large for one CU: every even 5-smooth size
from 136 to 960 runs the planned large-patch pipeline (csrc/pc_large_kernel.hip) with that model's L6 - L8, against the oracle's
double evaluation of the model (tests/oracle_lib.py, fft_process_ocl).

Bars: 1e-4 px on clear-peak patches (second-highest surface value below half the peak, from the f64 oracle's diagnostics); the NaN
pattern equals the oracle's on every patch.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import FftMethod, MofError, _capi, release_captured, synth
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu
TOL = 1e-4
BIN = os.path.join(os.path.dirname(__file__), "cpp", "test_processors")


def _check(got, cur, prev, lay, sr=55, label=""):
    """got [patches, 2] against the f64 oracle: NaN pattern everywhere, 1e-4 px on clear peaks. Returns the patches pinned."""
    want, _, diags = O.fft_process_ocl(cur, prev, lay, sr, 64, want_diag=True)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, got, want)
    n = 0
    for p in range(want.shape[0]):
        d = diags[p]
        if np.isfinite(d.peak_value) and d.second_value < 0.5 * d.peak_value:
            assert np.allclose(got[p], want[p], rtol=0, atol=TOL, equal_nan=True), (label, p, got[p], want[p])
            n += 1
    return n


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _translated(k, n, dx, dy):
    """(cur, prev) n x n crops of one texture, cur = prev moved by (dx, dy) as synth.pair_np plants it -- beyond pair_np's margin"""
    r = 100
    c = synth.canvas_np(k, n + 2 * r, n + 2 * r, True)
    o = synth.MARGIN + r
    return c[o - dy:o - dy + n, o - dx:o - dx + n].copy(), c[o:o + n, o:o + n].copy()


SIZES = [144, 150, 160, 180, 192, 200, 216, 240, 250, 256, 300, 320, 360, 384, 400, 432, 480, 500, 512, 540, 600, 640, 720, 750, 768,
         810, 960]  # (750, 810: the stage routine with one body per radix; 200 ... 480 include the estimator's tuned transform sizes)


@pytest.mark.parametrize("n", SIZES)
def test_ocl_large_patches_match_oracle(gpu, n):
    gx, gy = (2, 2) if n <= 256 else (1, 1)
    stride = (n + 5, n + 2)
    w, h = 3 + stride[0] * (gx - 1) + n + 4, 2 + stride[1] * (gy - 1) + n + 3
    B = 4 if n < 512 else 1  # (the f64 oracle is the slow part at the largest sizes)
    cur, prev, shifts, kinds = synth.batch_np(B, h, w, min(n // 8, 24), k0=n)
    fm = FftMethod(sample_point_size=n, frame_shape=(h, w), grid=(gx, gy), origin=(3, 2), stride=stride, peak_model=PEAK_OCL)
    assert fm.kernel_variant == "planned-large"
    got = fm.process_batch_device(_dev(cur, gpu), _dev(prev, gpu)).cpu().numpy()
    lay = O.fft_layout(w, h, n, gx, gy, (3, 2), stride)
    checked = sum(_check(got[k], cur[k], prev[k], lay, 55, f"n{n}/pair{k}/{kinds[k]}") for k in range(B))
    assert checked >= 0.5 * B * gx * gy, (n, checked)
    for k in range(B):
        if kinds[k] == "shift":
            assert np.allclose(np.nanmedian(got[k], axis=0), shifts[k], rtol=0, atol=0.5), (n, k, got[k], shifts[k])
    # one pair alone (a pass of one frame pair through the scratch) gives the same bits
    k = B - 1
    one = fm.process_batch_device(_dev(cur[k:k + 1], gpu), _dev(prev[k:k + 1], gpu)).cpu().numpy()
    assert np.array_equal(one[0], got[k], equal_nan=True)


def _run_cpp(args, frames, tmp_path):
    assert os.path.exists(BIN), "tests/cpp/test_processors missing: run __graft_entry__.build()"
    path = tmp_path / "frames.raw"
    frames.tofile(path)
    out = subprocess.run([BIN] + [str(a) for a in args] + [str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return [line.split() for line in out.stdout.strip().splitlines()]


@pytest.mark.parametrize("fs,sps", [(480, 160), (480, 240), (480, 480), (480, 100), (450, 150), (400, 200)])
def test_ocl_large_reference_constructor_stateful(gpu, tmp_path, fs, sps):
    """FftMethod(frameSize, samplePointSize, .., peak_model) as the node constructs it under useOCL=true; 480 / 100 is the reference's
    fallback to one 480 x 480 patch (FftMethod.cpp:1709-1716)."""
    fm = FftMethod(fs, sps, 80.0, peak_model=PEAK_OCL)
    n = sps if fs % sps == 0 else fs
    sq = fs // n
    assert fm.cfg.patch_size == n and fm.sqNum == sq and fm.kernel_variant == "planned-large"
    frames = np.stack([synth.pair_np(11 + sps, fs, fs, 3 * t, -2 * t, blur=True)[0] for t in range(3)])
    lay = O.fft_layout(fs, fs, n, sq, sq)
    out0 = fm.processImage(frames[0])  # the first frame correlates with itself (FftMethod.cpp:1761)
    assert _check(out0, frames[0], frames[0], lay, 55, "self") == sq * sq
    assert np.allclose(out0, 0.0, rtol=0, atol=TOL)
    for t in (1, 2):
        out = fm.processImage(frames[t])
        assert _check(out, frames[t], frames[t - 1], lay, 55, f"fs{fs}/n{sps}/t{t}") >= max(1, sq * sq - 1)
    if (fs, sps) == (480, 100):  # the C++ constructor the node uses (include/mof/processors.hpp)
        lines = _run_cpp(["fftocl", fs, sps, 80, 3], frames, tmp_path)
        assert len(lines) == 3
        for t, tok in enumerate(lines):
            assert tok[0] == "frame" and int(tok[1]) == t and int(tok[3]) == 1
            got = np.array([float(v) for v in tok[4:]]).reshape(1, 2)
            want, _ = O.fft_process_ocl(frames[t], frames[t - 1] if t else frames[t], lay, 55, 64)
            assert np.allclose(got, want, rtol=0, atol=TOL, equal_nan=True), (t, got, want)


def test_ocl_large_refuses_what_the_reference_cannot_plan(gpu):
    with pytest.raises(MofError) as exc:
        FftMethod(470, 100, 80.0, peak_model=PEAK_OCL)  # one 470 x 470 patch: 470 = 2 * 5 * 47
    assert exc.value.code == _capi.MOF_ERR_UNSUPPORTED
    assert FftMethod(470, 100, 80.0).kernel_variant == "planned-large"  # (cv::phaseCorrelate pads it to 480)


def test_ocl_large_model_specifics(gpu):
    """n = 240: the +-search_radius mask, constant patches, identical frames, and what search_radius changes."""
    n = 240
    tex = synth.canvas_np(9, n, n, False)[:n, :n].copy()
    lay = O.fft_layout(n, n, n, 1, 1)
    fm = FftMethod(n, n, 80.0, peak_model=PEAK_OCL)  # search_radius 55
    assert fm.kernel_variant == "planned-large"
    for dx, dy in ((20, -30), (-41, 7), (53, -50)):  # circular shifts inside the radius: found, exact integers
        cur = np.roll(tex, (dy, dx), axis=(0, 1))
        got = fm.process_batch_host(cur[None], tex[None])[0]
        assert _check(got, cur, tex, lay, 55, f"shift{dx},{dy}") == 1
        assert np.allclose(got, [[dx, dy]], rtol=0, atol=TOL), (dx, dy, got)
    # translations beyond it are masked: the maximum is taken from what is left of the surface, never the planted shift (translated
    # crops, not circular shifts: what is left is the texture's own correlation, not rounding noise, so the oracle pins it)
    for k, (dx, dy) in enumerate(((70, 0), (0, -90), (62, 61))):
        cur, prev = _translated(40 + k, n, dx, dy)
        got = fm.process_batch_host(cur[None], prev[None])[0]
        _check(got, cur, prev, lay, 55, f"masked{dx},{dy}")
        assert np.all(np.isnan(got)) or not np.allclose(got, [[dx, dy]], rtol=0, atol=1.0), (dx, dy, got)
        wide = FftMethod(n, n, 200.0, peak_model=PEAK_OCL, search_radius=100).process_batch_host(cur[None], prev[None])[0]
        assert _check(wide, cur, prev, O.fft_layout(n, n, n, 1, 1, max_px_speed=200.0), 100, f"wide{dx},{dy}") == 1
        assert np.allclose(wide, [[dx, dy]], rtol=0, atol=0.5), (dx, dy, wide)
    # constant patches: 1 / 0 in the real-only slots -> NaN, against texture or each other; identical frames -> (0, 0)
    const = np.full((n, n), 200, np.uint8)
    for c, p in ((const, tex), (tex, const), (const, const)):
        got = fm.process_batch_host(c[None], p[None])[0]
        assert np.isnan(got).all() and np.isnan(O.fft_process_ocl(c, p, lay)[0]).all()
    assert np.allclose(fm.process_batch_host(tex[None], tex[None])[0], [[0.0, 0.0]], rtol=0, atol=TOL)
    # search_radius: each radius matches the oracle at that radius; where the oracle gives the same answer for two radii, the engine
    # gives the same bits
    planted = ((-25, 11), (-18, 24), (-11, 37), (-4, -31))
    B = len(planted)
    pairs = [_translated(60 + k, n, dx, dy) for k, (dx, dy) in enumerate(planted)]
    cur, prev = np.stack([c for c, _ in pairs]), np.stack([p for _, p in pairs])
    got = {}
    for sr in (20, 55, 100):
        f = FftMethod(n, n, 80.0, peak_model=PEAK_OCL, search_radius=sr)
        got[sr] = f.process_batch_device(_dev(cur, gpu), _dev(prev, gpu)).cpu().numpy()
        for k in range(B):
            _check(got[sr][k], cur[k], prev[k], lay, sr, f"sr{sr}/pair{k}")
    for k in range(B):
        want = {sr: O.fft_process_ocl(cur[k], prev[k], lay, sr, 64)[0] for sr in got}
        for a, b in ((20, 55), (55, 100)):
            if np.array_equal(want[a], want[b], equal_nan=True):
                assert np.array_equal(got[a][k], got[b][k], equal_nan=True), (k, a, b)
    assert not np.array_equal(got[20], got[55], equal_nan=True)  # (shifts beyond 20 px: the narrow radius masks them)
    assert np.allclose(got[55][:, 0], planted, rtol=0, atol=0.5)


@pytest.mark.parametrize("n", [200, 480])
def test_ocl_large_entries_agree(gpu, n):
    """Device batch = host batch; BGR8 = gray on rgb2gray of the same frames; sequence = pairs of consecutive frames; a HIP-graph
    capture of the batch entry replays to the eager bits."""
    gx, gy = (2, 1) if n == 200 else (1, 1)
    w, h = 3 + (n + 4) * (gx - 1) + n + 2, n + 5
    B = 3
    rng = np.random.default_rng(n)
    video_bgr = np.stack([np.roll(synth.canvas_np(5, h + 64, w + 64, True)[:h, :w], (t, -2 * t), axis=(0, 1)) for t in range(B + 1)])
    video_bgr = np.stack([video_bgr, 255 - video_bgr // 2, (video_bgr // 4 * 3 + rng.integers(0, 20, video_bgr.shape)).astype(np.uint8)],
                         axis=-1).astype(np.uint8)
    video = np.stack([O.rgb2gray(f) for f in video_bgr])
    fm = FftMethod(sample_point_size=n, frame_shape=(h, w), grid=(gx, gy), origin=(3, 2), stride=(n + 4, 1), peak_model=PEAK_OCL)
    assert fm.kernel_variant == "planned-large"
    cur, prev = video[1:], video[:-1]
    dev = fm.process_batch_device(_dev(cur, gpu), _dev(prev, gpu)).cpu().numpy()
    lay = O.fft_layout(w, h, n, gx, gy, (3, 2), (n + 4, 1))
    assert sum(_check(dev[k], cur[k], prev[k], lay, 55, f"n{n}/pair{k}") for k in range(B)) >= B * gx * gy - 1
    host = fm.process_batch_host(cur, prev)
    assert np.array_equal(host, dev, equal_nan=True)
    bgr = fm.process_batch_device_bgr(_dev(video_bgr[1:], gpu), _dev(video_bgr[:-1], gpu)).cpu().numpy()
    assert np.array_equal(bgr, dev, equal_nan=True)
    seq = fm.process_sequence_device(_dev(video, gpu)).cpu().numpy()
    assert np.array_equal(seq, dev, equal_nan=True)
    # graph capture: a warm-up batch of this size has sized the scratch (above)
    tc, tp = _dev(cur, gpu), _dev(prev, gpu)
    want = fm.process_batch_device(tc, tp).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fm.process_batch_device(tc, tp)
    out.zero_()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    del g
    release_captured(fm)


def test_ocl_large_long_range(gpu):
    """The long-range mode (FftMethod.cpp:1931-1932) on the reference's tiling of a 2304 x 2304 frame into 144 x 144 patches: 4 x 4
    quarter-resolution patches of 144 pixels, against the oracle on resize_quarter of both frames."""
    fs, n = 2304, 144
    fm = FftMethod(fs, n, 80.0, peak_model=PEAK_OCL)
    assert fm.sqNum == 16 and fm.kernel_variant == "planned-large"
    cur, prev = synth.pair_np(n, fs, fs, 16, -28, blur=True)
    out = fm.process_long_range_batch_device(_dev(cur[None], gpu), _dev(prev[None], gpu)).cpu().numpy()[0]
    qc, qp = O.resize_quarter(cur), O.resize_quarter(prev)
    assert _check(out, qc, qp, O.fft_layout(fs // 4, fs // 4, n, 4, 4), 55, "long-range") >= 12
    assert np.allclose(np.nanmedian(out, axis=0), [4, -7], rtol=0, atol=0.5)
