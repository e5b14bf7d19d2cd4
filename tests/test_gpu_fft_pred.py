"""GPU tests of the FFT engine's predicted-shift window offsets and its coarse-to-fine entry (include/mof.h, "Predicted-shift window
offsets"; csrc/pc_offset_kernel.hip). Inputs, layouts (one per pair route) and the numpy restatements of the definitions:
tests/pred_cases.py; what the CPU oracle says about those inputs: tests/test_fft_pred_host.py.

Reference for the bits: the engine's PLAIN batch entry -- held to the CPU oracle by the shift and quality tests -- on a previous frame
whose windows torch gathered at the applied predictions. Reference for the values: tests/tolerances.py against the CPU oracle on the two
windows, nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle_lib as O
import pred_cases as PC
import tolerances as T
from mrs_optic_flow_amd import FftMethod, MofError, _capi, release_captured, synth
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu
NAMES = [l.name for l in PC.LAYOUTS + PC.EDGE_LAYOUTS]  # (the edge layouts: the sizes the window-offset kernels branch on)


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _zero(shifts):
    """a frame against itself: the zero shift, at the bar of tests/tolerances.py (the oracle of identical windows returns 0 to ~1e-7)"""
    return bool(np.abs(shifts).max() <= T.TOL)


def _frames(l, arr, gpu):
    """[n, H, W] uint8 on the device with the layout's row pitch (a view into [n, H, pitch] of 0xAB bytes)"""
    t = torch.full((arr.shape[0], l.h, l.pitch), 0xAB, dtype=torch.uint8, device=gpu)
    v = t[:, :, :l.w]
    v.copy_(torch.tensor(arr, device=gpu))
    return v


def _engine(l, **kw):
    args = PC.engine_kwargs(l)
    args.update(kw)
    fm = FftMethod(**args)
    if "peak_model" not in kw:
        assert fm.kernel_variant == l.variant, (l.name, fm.kernel_variant)
    return fm


def _gather_torch(l, prev, applied):
    """the displaced previous frames, gathered by torch on the device: window (x0, y0) <- window (x0 - a_x, y0 - a_y)"""
    out = torch.zeros((prev.shape[0], l.h, prev.stride(1)), dtype=torch.uint8, device=prev.device)[:, :, :l.w]  # (prev's row pitch)
    for k in range(prev.shape[0]):
        for p in range(applied.shape[1]):
            x0, y0 = PC.origin_of(l, p)
            ax, ay = (int(v) for v in applied[k, p])
            out[k, y0:y0 + l.n, x0:x0 + l.n] = prev[k, y0 - ay:y0 - ay + l.n, x0 - ax:x0 - ax + l.n]
    return out


# ---- 2. zero prediction ----
@pytest.mark.parametrize("name", NAMES)
def test_zero_prediction_has_the_plain_entrys_bits(gpu, name):
    c = PC.case(name)
    l = c.layout
    fm = _engine(l)
    cur, prev = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu)
    zeros = torch.zeros((PC.N_PAIRS, PC.patches(l), 2), dtype=torch.int32, device=gpu)
    want, want_q = fm.process_batch_device(cur, prev, return_quality=True)
    got, got_q, applied = fm.process_batch_device_pred(cur, prev, zeros, return_quality=True, return_applied=True)
    bare = fm.process_batch_device_pred(cur, prev, zeros)
    torch.cuda.synchronize()
    assert not np.isnan(_np(want)).any()
    assert _same_bits(got, want) and _same_bits(got_q, want_q) and _same_bits(bare, want)
    assert not _np(applied).any()


# ---- 3. bit-identity with a displaced frame built by torch ----
@pytest.mark.parametrize("name", NAMES)
def test_offset_windows_have_the_bits_of_a_gathered_frame(gpu, name):
    c = PC.case(name)
    l = c.layout
    fm = _engine(l)
    cur, prev = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu)
    pred = torch.tensor(c.pred, device=gpu)
    helper = np.array([[fm.pred_clamp(p, *c.pred[k, p]) for p in range(PC.patches(l))] for k in range(PC.N_PAIRS)])
    assert np.array_equal(helper, c.applied)
    got, got_q, applied = fm.process_batch_device_pred(cur, prev, pred, return_quality=True, return_applied=True)
    bare = fm.process_batch_device_pred(cur, prev, pred)
    disp = _gather_torch(l, prev, helper)
    assert np.array_equal(_np(disp)[:, :, :l.w], c.disp)
    plain, plain_q = fm.process_batch_device(cur, disp, return_quality=True)
    torch.cuda.synchronize()
    assert applied.dtype == torch.int32 and np.array_equal(_np(applied), helper)
    want = PC.total_np(helper, _np(plain))
    assert not np.isnan(want).any()
    assert _same_bits(got, want), np.argwhere(_bits(got) != _bits(want)).tolist()[:8]
    assert _same_bits(got_q, plain_q) and _same_bits(bare, got)
    assert _same_bits(_np(prev), c.prev) and _same_bits(_np(cur), c.cur)  # the caller's frames are read only


# ---- 4. oracle ----
@pytest.mark.parametrize("name", NAMES)
def test_residuals_against_the_oracle(gpu, name):
    """got - applied against -O.phase_correlate(cur window, displaced prev window) at 64 and 32 bit, every patch, by the rule of
    tests/tolerances.py alone (at n = 8 the patches without a clear peak are left out: at most pred_cases.unclear_cap, none elsewhere)"""
    c = PC.case(name)
    l = c.layout
    fm = _engine(l)
    got, applied = fm.process_batch_device_pred(_frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu), return_applied=True)
    got, applied = _np(got), _np(applied)
    assert np.array_equal(applied, c.applied)
    w64, w32, clear = PC.residual_oracles(name)
    left_out = int((~clear).sum())
    assert left_out <= PC.unclear_cap(name)  # (0 everywhere but at n = 8)
    worst = 0.0
    for k in range(PC.N_PAIRS):
        for p in range(PC.patches(l)):
            if not clear[k, p]:
                continue
            r = got[k, p] - applied[k, p]
            worst = max(worst, float(np.abs(r - w64[k, p]).max()))
            pinned = T.check_patch(r, w64[k, p], w32[k, p], f"pred/{name}/pair{k}", p, what="offset window",
                                   pixels=(PC.window(l, c.cur[k], p), PC.window(l, c.disp[k], p)))
            assert pinned, (name, k, p)
    print(f"{name}: worst |residual - f64 oracle| = {worst:.3g} px over {PC.N_PAIRS * PC.patches(l) - left_out} patches, {left_out} left out")


# ---- 5. coarse to fine ----
@pytest.mark.parametrize("fs", sorted(PC.C2F))
def test_coarse_to_fine(gpu, fs):
    l, cur_np, prev_np, coarse64, coarse32 = PC.c2f_case(fs)
    planted = np.array(PC.C2F[fs], np.float64)
    fm = _engine(l)
    cur, prev = _frames(l, cur_np, gpu), _frames(l, prev_np, gpu)
    got, quality, applied, coarse = (_np(t) for t in fm.process_coarse_to_fine_batch_device(cur, prev, return_quality=True, return_applied=True,
                                                                                           return_coarse=True))
    plain = _np(fm.process_batch_device(cur, prev))
    lr = _np(fm.process_long_range_batch_device(cur, prev))
    assert _same_bits(coarse, lr)
    # the long-range shifts, by the tolerance rule, on the quarter-resolution patches
    n_lr = coarse.shape[1]
    gxl = l.grid[0] // 4
    for k in range(2):
        qc, qp = O.resize_quarter(cur_np[k]), O.resize_quarter(prev_np[k])
        for p in range(n_lr):
            x0, y0 = (p % gxl) * l.n, (p // gxl) * l.n
            assert T.check_patch(coarse[k, p], coarse64[k, p], coarse32[k, p], f"pred/c2f{fs}/coarse{k}", p, what="long-range pass",
                                 pixels=(qc[y0:y0 + l.n, x0:x0 + l.n], qp[y0:y0 + l.n, x0:x0 + l.n]))
    # predictions: mof_fft_pred_from_coarse of the device's long-range shifts, which is the oracle's prediction
    pred = PC.c2f_pred_np(l, coarse)
    lib = _capi.load()
    for k in range(2):
        for p in range(n_lr):
            px, py = C.c_int32(0), C.c_int32(0)
            assert lib.mof_fft_pred_from_coarse(coarse[k, p, 0], coarse[k, p, 1], C.byref(px), C.byref(py)) == 0
            assert (px.value, py.value) == PC.round4_np(*coarse[k, p]) == PC.round4_np(*coarse64[k, p])
    assert np.array_equal(applied, PC.applied_np(l, pred))
    # pair 1 is an identical pair: prediction 0, the plain entry's bits
    assert not applied[1].any() and _same_bits(got[1], plain[1])
    # pair 0: the composition on the displaced windows
    disp = PC.displaced_np(l, prev_np, applied)
    free = (applied[0] == pred[0]).all(axis=-1)
    n_clamped, may_skip = PC.C2F_MAX_LEFT_OUT[fs]
    assert int((~free).sum()) == n_clamped
    skipped, worst = 0, 0.0
    for p in range(PC.patches(l)):
        a, b = PC.window(l, cur_np[0], p), PC.window(l, disp[0], p)
        (x64, y64), d = O.phase_correlate(a, b, 64)
        (x32, y32), _ = O.phase_correlate(a, b, 32)
        clear = d["second_value"] < 0.5 * d["peak_value"]
        if not clear:
            assert not free[p], ("a patch whose clamp is inactive must have a clear peak", p)
            skipped += 1
            continue
        assert T.check_patch(got[0, p] - applied[0, p], (-x64, -y64), (-x32, -y32), f"pred/c2f{fs}/fine", p, what="coarse to fine", pixels=(a, b)), p
        if free[p]:
            worst = max(worst, float(np.abs(got[0, p] - planted).max()))
    assert worst <= 0.25, worst
    assert skipped <= may_skip, skipped
    # the ground this adds: the plain entry cannot measure this shift
    wrong = ~(np.abs(plain[0] - planted).max(axis=-1) <= 0.5)
    assert wrong.sum() * 2 >= PC.patches(l), int(wrong.sum())
    print(f"frame {fs}: plain wrong on {int(wrong.sum())} of {PC.patches(l)}; coarse to fine: worst free patch {worst:.3f} px from the planted shift, "
          f"{skipped} of {n_clamped} clamped patches left out")


# ---- 6. gates ----
def test_speed_gate_acts_on_the_total(gpu):
    """max_px_speed = 3 with a planted (4, -3) predicted exactly: the interior residuals are ~0 and pass, the totals are 5 px and fail"""
    c = PC.case("k1_32")
    l = c.layout
    fm = _engine(l, max_px_speed=3.0)
    cur, prev = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu)
    pred_np = np.broadcast_to(c.planted[:, None, :], c.pred.shape).astype(np.int32)
    applied = PC.applied_np(l, pred_np)
    got = _np(fm.process_batch_device_pred(cur, prev, torch.tensor(np.ascontiguousarray(pred_np), device=gpu)))
    residual = _np(fm.process_batch_device(cur, torch.tensor(PC.displaced_np(l, c.prev, applied), device=gpu)))
    want = PC.total_np(applied, residual, 3.0)
    assert _same_bits(got, want)
    free = (applied == pred_np).all(axis=-1)
    assert free.sum() >= 8 and not np.isnan(residual[free]).any() and np.isnan(got[free]).all()
    assert np.array_equal(np.isnan(got[..., 0]), np.isnan(got[..., 1]))


def test_speed_gate_counts_in_n_invalid(gpu):
    """the stateful entry: with max_px_speed = 10 the coarse shift and the residuals pass and the totals of (24, -20) fail"""
    l, cur_np, prev_np, _, _ = PC.c2f_case(128)
    outs = {}
    for speed in (80.0, 10.0):
        fm = _engine(l, max_px_speed=speed)
        assert _zero(fm.process_image_coarse_to_fine(prev_np[0])) and fm.last_invalid == 0
        outs[speed] = fm.process_image_coarse_to_fine(cur_np[0])
        assert fm.last_invalid == int(np.isnan(outs[speed][:, 0]).sum())
    far = np.hypot(outs[80.0][:, 0], outs[80.0][:, 1]) > 10.0
    assert far.sum() >= 9 and np.isnan(outs[10.0][far]).all()


def test_response_gate_keeps_the_bits_of_what_passes(gpu):
    c = PC.case("k1_32")
    l = c.layout
    fm = _engine(l)
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    s0, q0 = (_np(t) for t in fm.process_batch_device_pred(cur, prev, pred, return_quality=True))
    v = float(np.median(q0[..., 0]))
    fm.set_min_response(v)
    s1, q1 = (_np(t) for t in fm.process_batch_device_pred(cur, prev, pred, return_quality=True))
    bare = _np(fm.process_batch_device_pred(cur, prev, pred))
    gated = ~(q0[..., 0] >= v)
    want = s0.copy()
    want[gated] = np.nan
    assert 0 < gated.sum() < gated.size
    assert _same_bits(s1, want) and _same_bits(q1, q0) and _same_bits(bare, s1)
    # coarse to fine: the gate acts on the coarse pass too -- a threshold above every response predicts 0 everywhere and gates every patch
    l2, cur_np, prev_np, _, _ = PC.c2f_case(128)
    f2 = _engine(l2, min_response=2.0)
    out, applied, coarse = (_np(t) for t in f2.process_coarse_to_fine_batch_device(_frames(l2, cur_np, gpu), _frames(l2, prev_np, gpu),
                                                                                  return_applied=True, return_coarse=True))
    assert np.isnan(coarse).all() and not applied.any() and np.isnan(out).all()


# ---- 7. the stateful entry ----
def test_stateful_entry_follows_the_frame_chain(gpu):
    l, cur_np, prev_np, _, _ = PC.c2f_case(128)
    f0, f1 = prev_np[0], cur_np[0]
    f2 = synth.pair_np(3, 128, 128, -9, 14)[0]  # (the same canvas, another window)
    fm, batch = _engine(l), _engine(l)

    def pair(cur, prev):
        out, q = batch.process_coarse_to_fine_batch_device(_frames(l, cur[None], gpu), _frames(l, prev[None], gpu), return_quality=True)
        return _np(out)[0], _np(q)[0]

    first = fm.process_image_coarse_to_fine(f0)
    assert _zero(first) and fm.last_invalid == 0
    for cur, prev in ((f1, f0), (f2, f1), (f2, f2), (f0, f2)):  # the chain advances on every call
        got = fm.process_image_coarse_to_fine(cur)
        want, want_q = pair(cur, prev)
        assert _same_bits(got, want) and _same_bits(fm.last_quality, want_q)
        assert fm.last_invalid == int(np.isnan(want[:, 0]).sum())
    fm.reset()
    assert _zero(fm.process_image_coarse_to_fine(f1))  # after reset the first frame meets itself ...
    assert _same_bits(fm.process_image_coarse_to_fine(f2), pair(f2, f1)[0])  # ... and becomes the previous one
    # the chain is processImage's own
    assert _same_bits(fm.processImage(f0), _np(batch.process_batch_device(_frames(l, f0[None], gpu), _frames(l, f2[None], gpu)))[0])
    assert _same_bits(fm.process_image_coarse_to_fine(f1), pair(f1, f0)[0])


# ---- 8. errors ----
def test_limits_return_their_codes_and_launch_nothing(gpu):
    lib = _capi.load()
    UNSUP, BAD = _capi.MOF_ERR_UNSUPPORTED, _capi.MOF_ERR_BAD_ARG
    l = PC.BY_NAME["k1_32"]
    c = PC.case("k1_32")
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    n, pt = PC.N_PAIRS, PC.patches(l)

    def sentinels(patches):
        return (torch.full((n, patches, 2), 7.0, dtype=torch.float64, device=gpu), torch.full((n, patches, 2), 7.0, dtype=torch.float64, device=gpu),
                torch.full((n, patches, 2), 7, dtype=torch.int32, device=gpu), torch.full((n, 1, 2), 7.0, dtype=torch.float64, device=gpu))

    def untouched(ts):
        torch.cuda.synchronize()
        return all(bool((t == 7).all()) for t in ts)

    def call_pred(fm, ts, cur=cur, prev=prev, pred=pred, pitch=None, out=True):
        return lib.mof_fft_process_batch_device_pred(fm._h, cur.data_ptr() if cur is not None else None, cur.stride(0) if cur is not None else 0,
                                                     prev.data_ptr() if prev is not None else None, prev.stride(0) if prev is not None else 0,
                                                     l.pitch if pitch is None else pitch, n, pred.data_ptr() if pred is not None else None,
                                                     ts[0].data_ptr() if out else None, ts[1].data_ptr(), ts[2].data_ptr(), None)

    def call_c2f(fm, ts, cur=cur, prev=prev, pitch=None, out=True):
        return lib.mof_fft_process_coarse_to_fine_batch_device(fm._h, cur.data_ptr() if cur is not None else None, cur.stride(0) if cur is not None else 0,
                                                               prev.data_ptr() if prev is not None else None, prev.stride(0) if prev is not None else 0,
                                                               l.pitch if pitch is None else pitch, n, ts[0].data_ptr() if out else None,
                                                               ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(), None)

    def message():
        return lib.mof_last_error().decode()

    fm = _engine(l)
    ts = sentinels(pt)
    # null pointers and a small pitch: MOF_ERR_BAD_ARG
    for kw in (dict(cur=None), dict(prev=None), dict(pred=None), dict(out=False), dict(pitch=l.w - 1)):
        assert call_pred(fm, ts, **kw) == BAD, kw
        assert untouched(ts)
    assert "pitch" in message()
    for kw in (dict(cur=None), dict(prev=None), dict(out=False), dict(pitch=l.w - 1)):
        assert call_c2f(fm, ts, **kw) == BAD, kw
        assert untouched(ts)
    assert lib.mof_fft_reserve_pred(fm._h, -1) == BAD
    null = type("NullEngine", (), {"_h": None})
    assert lib.mof_fft_reserve_pred(None, 1) == call_pred(null, ts) == call_c2f(null, ts) == _capi.MOF_ERR_NOT_INIT and untouched(ts)
    assert call_pred(fm, ts) == 0 and not untouched(ts[:3])  # (the same call with every argument in place runs)
    # an overlapping layout (the BASELINE c2 / c4 kind): MOF_ERR_UNSUPPORTED on both entries
    over = FftMethod(sample_point_size=32, frame_shape=(128, 128), grid=(4, 4), origin=(0, 0), stride=(24, 24))
    ts = sentinels(16)
    assert call_pred(over, ts) == UNSUP and "overlap" in message() and untouched(ts)
    assert call_c2f(over, ts) == UNSUP and "overlap" in message() and untouched(ts)
    with pytest.raises(MofError) as exc:
        over.process_batch_device_pred(cur, prev, pred)
    assert exc.value.code == UNSUP
    # the OpenCL peak model
    ocl = _engine(l, peak_model=PEAK_OCL)
    assert call_pred(ocl, ts) == UNSUP and "MOF_PEAK_OCL" in message() and untouched(ts)
    assert call_c2f(ocl, ts) == UNSUP and "MOF_PEAK_OCL" in message() and untouched(ts)
    # coarse to fine off the reference tiling: an origin, and a grid under 4 x 4
    for name in ("offset_32", "k1_64"):
        lo = PC.BY_NAME[name]
        co = PC.case(name)
        fo = _engine(lo)
        tso = sentinels(PC.patches(lo))
        co_cur, co_prev = _frames(lo, co.cur, gpu), _frames(lo, co.prev, gpu)
        rc = lib.mof_fft_process_coarse_to_fine_batch_device(fo._h, co_cur.data_ptr(), co_cur.stride(0), co_prev.data_ptr(), co_prev.stride(0), lo.pitch, n,
                                                             tso[0].data_ptr(), tso[1].data_ptr(), tso[2].data_ptr(), tso[3].data_ptr(), None)
        assert rc == UNSUP and "long-range" in message() and untouched(tso), name
        out = np.full((PC.patches(lo), 2), 7.0)
        ninv = C.c_int(7)
        assert lib.mof_fft_process_coarse_to_fine(fo._h, co.cur[0].ctypes.data, lo.w, out.ctypes.data, None, C.byref(ninv)) == UNSUP
        assert (out == 7.0).all() and ninv.value == 7
    # the stateful entry's own arguments
    out = np.full((pt, 2), 7.0)
    assert lib.mof_fft_process_coarse_to_fine(fm._h, None, l.w, out.ctypes.data, None, None) == BAD
    assert lib.mof_fft_process_coarse_to_fine(fm._h, c.cur[0].ctypes.data, l.w - 1, out.ctypes.data, None, None) == BAD
    assert lib.mof_fft_process_coarse_to_fine(fm._h, c.cur[0].ctypes.data, l.w, None, None, None) == BAD
    assert (out == 7.0).all()


# ---- 9. capture ----
def test_capture_after_reserve_and_refusal_without(gpu):
    c = PC.case("k1_32")
    l = c.layout
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    side = torch.cuda.Stream()
    # a fresh engine would have to grow its scratch inside the capture: refused before anything is launched
    fresh = _engine(l)
    marker = torch.zeros(1, device=gpu)
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(refused, stream=side):
            marker.add_(1.0)  # (so that the refused call leaves no empty graph behind)
            with pytest.raises(MofError) as exc:
                fresh.process_batch_device_pred(cur, prev, pred)
    torch.cuda.synchronize()
    assert exc.value.code == _capi.MOF_ERR_BAD_ARG and "capture" in str(exc.value), str(exc.value)
    assert not fresh.graph_pinned
    del refused
    release_captured(fresh)
    # after reserve_pred: one single-stream capture, two replays, the eager bits
    fm = _engine(l)
    want, want_q, want_a = (t.clone() for t in _engine(l).process_batch_device_pred(cur, prev, pred, return_quality=True, return_applied=True))
    want_c = _engine(l).process_coarse_to_fine_batch_device(cur, prev).clone()
    fm.reserve_pred(PC.N_PAIRS)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            got, got_q, got_a = fm.process_batch_device_pred(cur, prev, pred, return_quality=True, return_applied=True)
            got_c = fm.process_coarse_to_fine_batch_device(cur, prev)
    assert fm.graph_pinned
    for _ in range(2):
        for t in (got, got_q, got_a, got_c):
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(got, want) and _same_bits(got_q, want_q) and _same_bits(got_a, want_a) and _same_bits(got_c, want_c)
    # pinned: a larger batch would move the scratch under the graph
    with pytest.raises(MofError) as exc:
        fm.process_batch_device_pred(cur.repeat(2, 1, 1), prev.repeat(2, 1, 1), pred.repeat(2, 1, 1))
    assert exc.value.code == _capi.MOF_ERR_BUSY and "graph" in str(exc.value)
    del graph
    release_captured(fm)
    assert not fm.graph_pinned
    assert _same_bits(fm.process_batch_device_pred(cur.repeat(2, 1, 1), prev.repeat(2, 1, 1), pred.repeat(2, 1, 1))[:PC.N_PAIRS], want)
