"""The cases of tests/test_gpu_fft_k1_finish.py, shared with tests/golden/make_k1_finish.py (which records what the library in use
computes for them). They walk what decides how a 64 x 64 patch ends in K1 (csrc/pc_kernel.hip): which wave holds the surface's maximum
(wave w owns the un-shifted columns [8 w, 8 w + 8) and those + 32), whether the maximum is attained in one wave or in several (flat and
periodic surfaces), where the 5 x 5 window is clamped, the validity gate, the quality output, and every one-patch form of the kernel.

A case is (name, run): run(g, dev) -> {key: numpy array}, g the dict of input arrays of the fixture (make_inputs). One 64 x 64 patch per
frame unless a case says otherwise; a pair is (cur, prev) = (the texture rolled by (dy, dx) with a tenth of its pixels redrawn, the
texture), so the surface is a peak at the roll over a noise floor and the window holds values that are not zero."""
import numpy as np

N = 64
# the peak column in each wave's columns, both halves, whichever sign the roll comes out with: 3 + 8 j and 64 - (3 + 8 j) cover w = 0 .. 3 twice
WAVE_ROLLS = [(dy, 3 + 8 * j) for j, dy in enumerate((2, 7, 11, 60, 55, 0, 21, 40))]
# shifted rows / columns 0, 1, 62, 63 are the un-shifted 32, 33, 30, 31 (and 34, for the other sign of a roll by 30)
EDGE = (30, 31, 32, 33, 34)
CLAMP_ROLLS = [(d, d) for d in EDGE] + [(d, 5) for d in EDGE[:4]] + [(6, d) for d in EDGE[:4]] + [(EDGE[i], EDGE[4 - i]) for i in (0, 1, 3, 4)]
GATE_ROLLS = [(0, 3), (2, 2), (3, 3), (0, 5), (5, 5), (-3, 1), (1, -4), (0, 0)]  # max_px_speed 4: |shift|^2 of 9, 8, 10, 0 pass; 18, 25, 50, 17 fail
OFFSET_PRED = np.array([[[5, -3]], [[-4, 6]], [[7, 2]], [[-2, -5]]], np.int32)


def _pair(rng, tex, dy, dx):
    cur = np.roll(tex, (dy, dx), axis=(0, 1)).copy()
    redraw = rng.random(tex.shape[:2]) < 0.1
    cur[redraw] = rng.integers(0, 256, cur[redraw].shape, dtype=np.uint8)
    return cur, tex


def _pairs(rng, rolls, shape=(N, N)):
    got = [_pair(rng, rng.integers(0, 256, shape, dtype=np.uint8), dy, dx) for dy, dx in rolls]
    return np.stack([c for c, _ in got]), np.stack([p for _, p in got])


def _ties(rng):
    """cur, prev [9, 64, 64]: 0 cur constant, 1 prev constant, 2 both constant, 3 both zero, 4 - 5 period 8 (equal maxima in every wave),
    6 - 7 period 32 (equal maxima in the two halves one wave owns), 8 period 16 along x only"""
    tex = rng.integers(0, 256, (N, N), dtype=np.uint8)
    cur, prev = np.stack([tex] * 9), np.stack([np.roll(tex, (1, 2), axis=(0, 1))] * 9)
    cur[0], prev[1], cur[2], prev[2], cur[3], prev[3] = 91, 200, 17, 240, 0, 0
    for k, (period_y, period_x, roll) in enumerate(((8, 8, (1, 2)), (8, 8, (0, 0)), (32, 32, (3, 1)), (32, 32, (0, 9)), (64, 16, (2, 5)))):
        t = np.tile(rng.integers(0, 256, (period_y, period_x), dtype=np.uint8), (N // period_y, N // period_x))
        cur[4 + k], prev[4 + k] = np.roll(t, roll, axis=(0, 1)), t
    return cur, prev


def make_inputs():
    rng = np.random.default_rng(20261022)
    g = {}
    g["wave_cur"], g["wave_prev"] = _pairs(rng, WAVE_ROLLS)
    g["clamp_cur"], g["clamp_prev"] = _pairs(rng, CLAMP_ROLLS)
    g["gate_cur"], g["gate_prev"] = _pairs(rng, GATE_ROLLS)
    g["tie_cur"], g["tie_prev"] = _ties(rng)
    g["bgr_cur"], g["bgr_prev"] = _pairs(rng, WAVE_ROLLS[::2] + CLAMP_ROLLS[1:2], (N, N, 3))
    # long-range mode: 256 x 256 frames of flat 2 x 2 blocks, one quarter-resolution patch of 64 x 64
    c, p = _pairs(rng, [(2 * dy, 2 * dx) for dy, dx in WAVE_ROLLS[1::4] + CLAMP_ROLLS[2:4]], (128, 128))
    g["lr_cur"], g["lr_prev"] = np.kron(c, np.ones((1, 2, 2), np.uint8)), np.kron(p, np.ones((1, 2, 2), np.uint8))
    # window offsets: one patch at (8, 8) of 80 x 80 frames, moved by the prediction
    g["off_cur"], g["off_prev"] = _pairs(rng, WAVE_ROLLS[:4], (80, 80))
    g["off_bgr_cur"], g["off_bgr_prev"] = _pairs(rng, WAVE_ROLLS[4:], (80, 80, 3))
    g["pred"] = OFFSET_PRED
    return g


def _np(t):
    return t.cpu().numpy()


def _dev(g, dev, *keys):
    import torch

    return [torch.from_numpy(g[k]).to(dev) for k in keys]


def _both_entries(plain, with_quality):
    """quality null and non-null: the default entry and the _q entry"""
    s, q = with_quality()
    return {"shift": _np(plain()), "shift_q": _np(s), "quality": _np(q)}


def _gray(what, max_px_speed=80.0):
    def run(g, dev):
        from mrs_optic_flow_amd import FftMethod

        fm = FftMethod(sample_point_size=N, max_px_speed=max_px_speed, frame_shape=(N, N), grid=(1, 1))
        assert fm.kernel_variant == "stockham", fm.kernel_variant
        cur, prev = _dev(g, dev, what + "_cur", what + "_prev")
        return _both_entries(lambda: fm.process_batch_device(cur, prev), lambda: fm.process_batch_device(cur, prev, return_quality=True))
    return run


def _bgr(g, dev):
    from mrs_optic_flow_amd import FftMethod

    fm = FftMethod(sample_point_size=N, frame_shape=(N, N), grid=(1, 1))
    cur, prev = _dev(g, dev, "bgr_cur", "bgr_prev")
    return _both_entries(lambda: fm.process_batch_device_bgr(cur, prev), lambda: fm.process_batch_device_bgr(cur, prev, return_quality=True))


def _long_range(g, dev):
    from mrs_optic_flow_amd import FftMethod

    fm = FftMethod(frame_size=256, sample_point_size=N)
    cur, prev = _dev(g, dev, "lr_cur", "lr_prev")
    return _both_entries(lambda: fm.process_long_range_batch_device(cur, prev),
                         lambda: fm.process_long_range_batch_device(cur, prev, return_quality=True))


def _offsets(bgr):
    def run(g, dev):
        from mrs_optic_flow_amd import FftMethod

        fm = FftMethod(sample_point_size=N, frame_shape=(80, 80), grid=(1, 1), origin=(8, 8))
        assert fm.pred_route_supported("fused")
        fm.set_pred_route("fused")
        cur, prev, pred = _dev(g, dev, *(("off_bgr_cur", "off_bgr_prev") if bgr else ("off_cur", "off_prev")), "pred")
        entry = fm.process_batch_device_pred_bgr if bgr else fm.process_batch_device_pred
        s, q, a = entry(cur, prev, pred, return_quality=True, return_applied=True)
        assert (_np(a) == g["pred"]).all(), _np(a).tolist()  # (non-zero offsets, none clamped)
        return {"shift": _np(entry(cur, prev, pred)), "shift_q": _np(s), "quality": _np(q)}
    return run


CASES = (("peak in each wave", _gray("wave")), ("several holders", _gray("tie")), ("clamped window", _gray("clamp", max_px_speed=1000.0)),
         ("gate", _gray("gate", max_px_speed=4.0)), ("bgr", _bgr), ("long range", _long_range),
         ("window offsets gray", _offsets(False)), ("window offsets bgr", _offsets(True)))
