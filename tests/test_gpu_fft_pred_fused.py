"""GPU tests of the FFT engine's FUSED window-offset route (include/mof.h, MOF_PRED_ROUTE_FUSED; csrc/pc_kernel.hip and
csrc/pc_half_kernel.hip with OFF on, csrc/pc_offset_kernel.hip's clamp kernel). Inputs and numpy restatements: tests/pred_cases.py and
tests/pred_fused_cases.py; what the CPU oracle says about the new inputs: tests/test_fft_pred_fused_host.py.

Reference for the bits: the gather route of the same engine wherever it runs, and -- on the overlapping layouts, which it cannot serve --
the engine's PLAIN entry on the unrolled frames (pred_fused_cases.unroll_np). Reference for the values: tests/tolerances.py against the
CPU oracle on the two windows, nothing else."""
import numpy as np
import pytest
import torch

import pred_cases as PC
import pred_fused_cases as F
import tolerances as T
from mrs_optic_flow_amd import FftMethod, MofError, _capi, release_captured
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu
# those of pred_cases.LAYOUTS with a fused form, and of its edge layouts: the padded and odd half-tile sizes (57 -> 60, 136 -> 144, 162)
FUSED_LAYOUTS = ["k1_32", "k1_64", "n120", "persistent_128", "k1h_96", "k1h_160", "offset_32"] + PC.EDGE_FUSED
OVER = [l.name for l in F.OVER]


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(a):
    a = np.ascontiguousarray(_np(a))
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _frames(l, arr, gpu):
    """[n, H, W] uint8 on the device with the layout's row pitch (a view into [n, H, pitch] of 0xAB bytes)"""
    t = torch.full((arr.shape[0], l.h, l.pitch), 0xAB, dtype=torch.uint8, device=gpu)
    v = t[:, :, :l.w]
    v.copy_(torch.tensor(arr, device=gpu))
    return v


def _engine(l, route="gather", **kw):
    args = PC.engine_kwargs(l)
    args.update(kw)
    fm = FftMethod(**args)
    if "peak_model" not in kw:
        assert fm.kernel_variant == l.variant, (l.name, fm.kernel_variant)
    assert fm.pred_route == "gather"  # every engine's default
    if route != "gather":
        fm.set_pred_route(route)
        assert fm.pred_route == route
    return fm


def _pred(fm, cur, prev, pred):
    return fm.process_batch_device_pred(cur, prev, pred, return_quality=True, return_applied=True)


# ---- 1. route against route ----
@pytest.mark.parametrize("name", FUSED_LAYOUTS)
def test_fused_route_has_the_gather_routes_bits(gpu, name):
    c = PC.case(name)
    l = c.layout
    fm = _engine(l)
    assert fm.pred_route_supported("fused") and fm.pred_route_supported("gather")
    cur, prev = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu)
    zeros = torch.zeros((PC.N_PAIRS, PC.patches(l), 2), dtype=torch.int32, device=gpu)
    plain, plain_q = fm.process_batch_device(cur, prev, return_quality=True)
    for pred in (torch.tensor(c.pred, device=gpu), zeros):
        want = _pred(fm, cur, prev, pred)
        fm.set_pred_route("fused")
        got = _pred(fm, cur, prev, pred)
        bare = fm.process_batch_device_pred(cur, prev, pred)
        fm.set_pred_route("gather")  # (back and forth on one engine, between calls)
        again = _pred(fm, cur, prev, pred)
        torch.cuda.synchronize()
        assert not np.isnan(_np(want[0])).any()
        for g, w, a in zip(got, want, again):
            assert _same_bits(g, w) and _same_bits(a, w), name
        assert _same_bits(bare, want[0])
        if pred is zeros:
            assert _same_bits(got[0], plain) and _same_bits(got[1], plain_q) and not _np(got[2]).any()
        else:
            assert np.array_equal(_np(got[2]), c.applied)
    assert _same_bits(_np(prev), c.prev) and _same_bits(_np(cur), c.cur)  # the caller's frames are read only


# ---- 2. overlapping layouts ----
@pytest.mark.parametrize("name", OVER)
def test_overlapping_layout_against_the_unrolled_frames_and_the_oracle(gpu, name):
    c = F.case(name)
    l, lu = c.layout, c.unrolled
    fm = _engine(l, "fused")
    cur, prev = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu)
    got, got_q, applied = (_np(t) for t in _pred(fm, cur, prev, torch.tensor(c.pred, device=gpu)))
    helper = np.array([[fm.pred_clamp(p, *c.pred[k, p]) for p in range(PC.patches(l))] for k in range(F.N_PAIRS)])
    assert np.array_equal(applied, helper) and np.array_equal(applied, c.applied)
    # the plain entry of an engine of layout L' on (cur', prev'): the kernels' arithmetic depends on the pixels, not on where the patch lies
    plain, plain_q = (_np(t) for t in _engine(lu).process_batch_device(_frames(lu, c.cur_u, gpu), _frames(lu, c.prev_u, gpu), return_quality=True))
    want = PC.total_np(applied, plain)
    assert not np.isnan(want).any()
    assert _same_bits(got, want), np.argwhere(_bits(got) != _bits(want)).tolist()[:8]
    assert _same_bits(got_q, plain_q)
    # the residuals against both oracles, every patch pinned
    w64, w32, clear = F.residual_oracles(name)
    assert clear.all()
    worst = 0.0
    for k in range(F.N_PAIRS):
        for p in range(PC.patches(l)):
            r = got[k, p] - applied[k, p]
            worst = max(worst, float(np.abs(r - w64[k, p]).max()))
            assert T.check_patch(r, w64[k, p], w32[k, p], f"pred_fused/{name}/pair{k}", p, what="fused offset window",
                                 pixels=(PC.window(lu, c.cur_u[k], p), PC.window(lu, c.prev_u[k], p))), (name, k, p)
    print(f"{name}: worst |residual - f64 oracle| = {worst:.3g} px over {F.N_PAIRS * PC.patches(l)} patches")
    # zero prediction: the plain entry on L itself
    zeros = torch.zeros((F.N_PAIRS, PC.patches(l), 2), dtype=torch.int32, device=gpu)
    z, z_q, z_a = _pred(fm, cur, prev, zeros)
    p0, p0_q = fm.process_batch_device(cur, prev, return_quality=True)
    assert _same_bits(z, p0) and _same_bits(z_q, p0_q) and not _np(z_a).any()
    assert _same_bits(_np(prev), c.prev) and _same_bits(_np(cur), c.cur)


# ---- 3. the persistent loop ----
def test_persistent_loop_rereads_the_offset_for_every_patch(gpu):
    """more patches than twice the resident workgroups: a workgroup reads the offset again for its second patch and for the prefetch of
    the patch after it; the predictions differ per patch"""
    c = PC.case("persistent_128")
    l = c.layout
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    n = (2 * cus) // PC.patches(l) + 3
    assert n * PC.patches(l) > 2 * cus
    reps = (n + PC.N_PAIRS - 1) // PC.N_PAIRS
    cur, prev = (_frames(l, np.tile(a, (reps, 1, 1))[:n], gpu) for a in (c.cur, c.prev))
    rng = np.random.RandomState(128)
    pred_np = rng.randint(-9, 10, size=(n, PC.patches(l), 2)).astype(np.int32)
    pred_np[-1, -1] = (PC.I32_MIN, PC.I32_MAX)  # (the launch's very last patch, clamped)
    assert len({tuple(v) for v in pred_np.reshape(-1, 2)}) > 100
    pred = torch.tensor(pred_np, device=gpu)
    fm = _engine(l)
    want = _pred(fm, cur, prev, pred)
    fm.set_pred_route("fused")
    got = _pred(fm, cur, prev, pred)
    torch.cuda.synchronize()
    for g, w in zip(got, want):
        assert _same_bits(g, w)
    assert np.array_equal(_np(got[2]), PC.applied_np(l, pred_np))
    assert not np.isnan(_np(got[0])).all()


# ---- 4. the pair split ----
def test_pair_split_advances_the_offsets(gpu):
    """65 540 pairs of one 32 x 32 patch: the launch goes out in two slices of pairs (65 535 + 5), non-zero predictions in the last five"""
    n = 65540
    fm = FftMethod(sample_point_size=32, max_px_speed=PC.SPEED, frame_shape=(40, 40), grid=(1, 1), origin=(4, 4), stride=(32, 32))
    assert fm.kernel_variant == "stockham"
    g = torch.Generator(device=gpu).manual_seed(32)
    prev = torch.randint(0, 256, (n, 40, 40), dtype=torch.uint8, device=gpu, generator=g)
    cur = torch.roll(prev, shifts=(1, 2), dims=(1, 2))  # content moved down 1, right 2
    pred_np = np.zeros((n, 1, 2), np.int32)
    pred_np[-5:, 0] = [(2, 1), (-3, 4), (4, -4), (PC.I32_MAX, PC.I32_MIN), (1, -2)]
    pred = torch.tensor(pred_np, device=gpu)
    want = _pred(fm, cur, prev, pred)
    fm.set_pred_route("fused")
    got = _pred(fm, cur, prev, pred)
    torch.cuda.synchronize()
    for g_, w in zip(got, want):
        assert _same_bits(g_, w)
    a = _np(got[2])
    assert not a[:-5].any() and a[-5:, 0].tolist() == [[2, 1], [-3, 4], [4, -4], [4, -4], [1, -2]]
    tail = _np(got[0])[-5:, 0]
    assert not np.isnan(tail[0]).any() and np.abs(tail[0] - (2, 1)).max() < 0.5  # (the last slice's first pair: predicted exactly)


# ---- 5. coarse to fine ----
@pytest.mark.parametrize("fs", sorted(PC.C2F))
def test_coarse_to_fine_on_both_routes(gpu, fs):
    l, cur_np, prev_np, _, _ = PC.c2f_case(fs)
    cur, prev = _frames(l, cur_np, gpu), _frames(l, prev_np, gpu)
    fm = _engine(l)
    kw = dict(return_quality=True, return_applied=True, return_coarse=True)
    want = fm.process_coarse_to_fine_batch_device(cur, prev, **kw)
    fm.set_pred_route("fused")
    got = fm.process_coarse_to_fine_batch_device(cur, prev, **kw)
    torch.cuda.synchronize()
    assert _np(want[2]).any() and not np.isnan(_np(want[0])).all()
    for g, w in zip(got, want):
        assert _same_bits(g, w)
    # the stateful entry over three frames
    outs = {}
    for route in ("gather", "fused"):
        f = _engine(l, route)
        outs[route] = [(f.process_image_coarse_to_fine(fr), f.last_quality, f.last_invalid) for fr in (prev_np[0], cur_np[0], prev_np[0])]
    for (a, aq, ai), (b, bq, bi) in zip(outs["gather"], outs["fused"]):
        assert _same_bits(a, b) and _same_bits(aq, bq) and ai == bi


# ---- 6. gates ----
def test_gates_act_alike_on_both_routes(gpu):
    c = PC.case("k1_32")
    l = c.layout
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    q0 = _np(_engine(l).process_batch_device_pred(cur, prev, pred, return_quality=True)[1])
    # the response gate at the median response, the speed gate at 3 px (planted: (4, -3) and (-3, 4): totals of 5 px)
    for kw, some in ((dict(min_response=float(np.median(q0[..., 0]))), True), (dict(max_px_speed=3.0), True), (dict(), False)):
        fm = _engine(l, **kw)
        want = [_np(t) for t in _pred(fm, cur, prev, pred)]
        fm.set_pred_route("fused")
        got = [_np(t) for t in _pred(fm, cur, prev, pred)]
        nan = np.isnan(want[0][..., 0])
        assert (nan.sum() > 0) == some and (not nan.all() or "max_px_speed" in kw), (kw, int(nan.sum()))
        assert np.array_equal(np.isnan(got[0][..., 0]), nan)
        for g, w in zip(got, want):
            assert _same_bits(g, w), kw
    # n_invalid, through the stateful entry (an armed response gate acts on both passes of coarse to fine)
    l2, cur_np, prev_np, _, _ = PC.c2f_case(128)
    counts = {}
    for route in ("gather", "fused"):
        f = _engine(l2, route, max_px_speed=10.0)
        f.process_image_coarse_to_fine(prev_np[0])
        out = f.process_image_coarse_to_fine(cur_np[0])
        counts[route] = (f.last_invalid, _bits(out).tolist())
        assert f.last_invalid == int(np.isnan(out[:, 0]).sum()) > 0
    assert counts["gather"] == counts["fused"]


# ---- 7. BGR8 ----
@pytest.mark.parametrize("name", ["k1_64", "n120", "over_128"])
def test_bgr_entry_has_the_gray_entrys_bits(gpu, name):
    c = F.case(name) if name in F.BY_NAME else PC.case(name)
    l = c.layout
    cur_bgr, prev_bgr = F.bgr_of(c.cur), F.bgr_of(c.prev)
    cur3, prev3 = torch.tensor(cur_bgr, device=gpu), torch.tensor(prev_bgr, device=gpu)
    cur1, prev1 = _frames(l, F.gray_of_bgr(cur_bgr), gpu), _frames(l, F.gray_of_bgr(prev_bgr), gpu)
    pred = torch.tensor(c.pred, device=gpu)
    fm = _engine(l)
    # the gather route: MOF_ERR_UNSUPPORTED, nothing launched
    lib = _capi.load()
    n, pt = c.pred.shape[0], PC.patches(l)
    ts = (torch.full((n, pt, 2), 7.0, dtype=torch.float64, device=gpu), torch.full((n, pt, 2), 7.0, dtype=torch.float64, device=gpu),
          torch.full((n, pt, 2), 7, dtype=torch.int32, device=gpu))
    rc = lib.mof_fft_process_batch_device_pred_bgr(fm._h, cur3.data_ptr(), cur3.stride(0), prev3.data_ptr(), prev3.stride(0), cur3.stride(1), n,
                                                   pred.data_ptr(), ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == _capi.MOF_ERR_UNSUPPORTED and "fused" in lib.mof_last_error().decode() and all(bool((t == 7).all()) for t in ts)
    with pytest.raises(MofError) as exc:
        fm.process_batch_device_pred_bgr(cur3, prev3, pred)
    assert exc.value.code == _capi.MOF_ERR_UNSUPPORTED
    fm.set_pred_route("fused")
    want = _pred(fm, cur1, prev1, pred)
    got = fm.process_batch_device_pred_bgr(cur3, prev3, pred, return_quality=True, return_applied=True)
    bare = fm.process_batch_device_pred_bgr(cur3, prev3, pred)
    torch.cuda.synchronize()
    assert not np.isnan(_np(want[0])).all() and np.array_equal(_np(got[2]), c.applied)
    for g, w in zip(got, want):
        assert _same_bits(g, w), name
    assert _same_bits(bare, want[0])
    # a pitch below three bytes per pixel is a bad argument
    rc = lib.mof_fft_process_batch_device_pred_bgr(fm._h, cur3.data_ptr(), cur3.stride(0), prev3.data_ptr(), prev3.stride(0), 3 * l.w - 1, n,
                                                   pred.data_ptr(), ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), None)
    assert rc == _capi.MOF_ERR_BAD_ARG


# ---- 8. limits ----
def test_limits_of_the_route_switch(gpu):
    lib = _capi.load()
    UNSUP, BAD, BUSY = _capi.MOF_ERR_UNSUPPORTED, _capi.MOF_ERR_BAD_ARG, _capi.MOF_ERR_BUSY
    # kernels without a fused form: the planned LDS kernel, the large-patch pipeline, the OpenCL peak model
    for fm in (_engine(PC.BY_NAME["planned_62"]), _engine(PC.BY_NAME["large_200"]), _engine(PC.BY_NAME["k1_32"], peak_model=PEAK_OCL)):
        assert lib.mof_fft_set_pred_route(fm._h, 1) == UNSUP and "fused" in lib.mof_last_error().decode()
        assert fm.pred_route == "gather" and not fm.pred_route_supported("fused")
        with pytest.raises(MofError) as exc:
            fm.set_pred_route("fused")
        assert exc.value.code == UNSUP and fm.pred_route == "gather"
    c = PC.case("k1_32")
    l = c.layout
    fm = _engine(l)
    for route in (2, -1):
        assert lib.mof_fft_set_pred_route(fm._h, route) == BAD and fm.pred_route == "gather"
    with pytest.raises(ValueError):
        fm.set_pred_route("scatter")
    # while a capture pins the engine: MOF_ERR_BUSY, the route unchanged
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    fm.reserve_pred(PC.N_PAIRS)
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            fm.process_batch_device_pred(cur, prev, pred)
    assert fm.graph_pinned
    assert lib.mof_fft_set_pred_route(fm._h, 1) == BUSY and "graph" in lib.mof_last_error().decode() and fm.pred_route == "gather"
    del graph
    release_captured(fm)
    fm.set_pred_route("fused")
    assert fm.pred_route == "fused"
    # a default engine: the overlapping layout is still MOF_ERR_UNSUPPORTED, and served once switched
    co = F.case("over_32")
    lo = co.layout
    over = _engine(lo)
    ocur, oprev, opred = _frames(lo, co.cur, gpu), _frames(lo, co.prev, gpu), torch.tensor(co.pred, device=gpu)
    with pytest.raises(MofError) as exc:
        over.process_batch_device_pred(ocur, oprev, opred)
    assert exc.value.code == UNSUP and "overlap" in str(exc.value)
    over.set_pred_route("fused")
    assert not np.isnan(_np(over.process_batch_device_pred(ocur, oprev, opred))).any()
    over.set_pred_route("gather")
    with pytest.raises(MofError) as exc:
        over.process_batch_device_pred(ocur, oprev, opred)
    assert exc.value.code == UNSUP


# ---- 9. capture ----
def test_capture_of_a_fused_call_and_no_displaced_frame_scratch(gpu):
    c = F.case("over_64")
    l = c.layout
    cur, prev, pred = _frames(l, c.cur, gpu), _frames(l, c.prev, gpu), torch.tensor(c.pred, device=gpu)
    live = _capi.load().mof_live_buffers
    want = [t.clone() for t in _pred(_engine(l, "fused"), cur, prev, pred)]
    torch.cuda.synchronize()
    base = live()
    fm = _engine(l, "fused")
    made = live() - base
    fm.reserve_pred(F.N_PAIRS)
    # the three per-pair side buffers (predictions, applied predictions, long-range shifts) and nothing else: no displaced frames
    assert live() - base == made + 3
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            got = _pred(fm, cur, prev, pred)
    assert fm.graph_pinned and live() - base == made + 3
    for _ in range(2):
        for t in got:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(got, want):
            assert _same_bits(g, w)
    del graph
    release_captured(fm)
    # the same engine design on the gather route holds one buffer more: the displaced frames (a layout the gather serves)
    l2 = PC.BY_NAME["k1_64"]
    counts = {}
    for route in ("fused", "gather"):
        b0 = live()
        f2 = _engine(l2, route)
        f2.reserve_pred(PC.N_PAIRS)
        counts[route] = live() - b0
        del f2
    assert counts["gather"] == counts["fused"] + 1, counts
