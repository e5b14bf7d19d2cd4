"""GPU tests of the coarse-to-fine PREDICTION MAP on fields it can get wrong, and of coarse to fine on every pair route (include/mof.h,
"Predicted-shift window offsets"; csrc/pc_offset_kernel.hip, pc_pred_from_coarse_kernel; csrc/mof_capi.hip, pred_run). Inputs:
tests/pred_field_cases.py; what the CPU oracles say about them, and the numpy proof that each wrong map would show:
tests/test_fft_pred_field_host.py.

Reference for the map: pred_cases.c2f_pred_np / applied_np on the device's long-range shifts AND on the f64 oracle's. For the bits: the
window-offset entry of a second engine fed those predictions, and the plain and long-range entries. For the values: tests/tolerances.py
against the CPU oracle on the two windows, nothing else."""
import numpy as np
import pytest
import torch

import pred_cases as PC
import pred_field_cases as FC
import tolerances as T
from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
NAMES = [l.name for l in FC.FIELDS]
ROUTES = ["gather", "fused"]
C2F = dict(return_quality=True, return_applied=True, return_coarse=True)


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


def _engine(l, route, **kw):
    args = PC.engine_kwargs(l)
    args.update(kw)
    fm = FftMethod(**args)
    assert fm.kernel_variant == l.variant, (l.name, fm.kernel_variant)
    if route != "gather":
        fm.set_pred_route(route)
    assert fm.pred_route == route
    return fm


def _pred_tensor(pred, gpu):
    return torch.tensor(np.ascontiguousarray(pred.astype(np.int32)), device=gpu)


def _coarse_and_map(fm, l, cur, prev, cur_np, prev_np, coarse64, coarse32, label):
    """C.1 and C.2: the coarse-to-fine entry's long-range shifts have the long-range entry's bits and are held to both oracles on the
    quarter-image patches; the applied predictions are the map of the device's shifts and of the f64 oracle's. Returns the numpy outputs
    and the predictions."""
    got, quality, applied, coarse = (_np(t) for t in fm.process_coarse_to_fine_batch_device(cur, prev, **C2F))
    assert _same_bits(coarse, fm.process_long_range_batch_device(cur, prev))
    for k in range(coarse.shape[0]):
        for c in range(coarse.shape[1]):
            assert T.check_patch(coarse[k, c], coarse64[k, c], coarse32[k, c], f"{label}/coarse{k}", c, what="long-range pass",
                                 pixels=lambda k=k, c=c: FC.lr_windows(l, cur_np[k], prev_np[k], c)), (k, c)
    pred = PC.c2f_pred_np(l, coarse)
    assert np.array_equal(applied, PC.applied_np(l, pred))
    assert np.array_equal(applied, PC.applied_np(l, PC.c2f_pred_np(l, coarse64)))
    return got, quality, applied, coarse, pred


def _composition(second, cur, prev, pred, got, quality, applied, gpu):
    """C.3: shifts, quality and applied predictions have the bits of the window-offset entry of a SECOND engine fed the predictions --
    every patch, no exclusions"""
    want, want_q, want_a = second.process_batch_device_pred(cur, prev, _pred_tensor(pred, gpu), return_quality=True, return_applied=True)
    torch.cuda.synchronize()
    assert _same_bits(got, want), np.argwhere(_bits(got) != _bits(want)).tolist()[:8]
    assert _same_bits(quality, want_q) and _same_bits(applied, want_a)


# ---- C.1 - C.5: piecewise shift fields ----
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_piecewise_field(gpu, name, route):
    s = FC.scene(name)
    l = s.layout
    fm, second = _engine(l, route), _engine(l, route)
    cur, prev = _frames(l, s.cur, gpu), _frames(l, s.prev, gpu)
    got, quality, applied, coarse, pred = _coarse_and_map(fm, l, cur, prev, s.cur, s.prev, s.coarse64, s.coarse32, f"pred_field/{name}/{route}")
    assert np.array_equal(pred, s.pred) and np.array_equal(applied, s.applied)
    _composition(second, cur, prev, pred, got, quality, applied, gpu)
    # 4. values: every inside patch, pinned
    worst = 0.0
    for k, p in np.argwhere(s.inside):
        r = got[k, p] - applied[k, p]
        worst = max(worst, float(np.abs(r - s.w64[k, p]).max()))
        assert T.check_patch(r, s.w64[k, p], s.w32[k, p], f"pred_field/{name}/{route}/pair{k}", p, what="coarse to fine",
                             pixels=(PC.window(l, s.cur[k], p), PC.window(l, s.disp[k], p))), (name, k, p)
    print(f"{name} ({route}): worst |residual - f64 oracle| = {worst:.3g} px over {int(s.inside.sum())} inside patches")
    # 5. the identical cell: prediction 0 and the plain entry's bits; no patch of another cell predicts 0 on either axis
    plain, plain_q = (_np(t) for t in fm.process_batch_device(cur, prev, return_quality=True))
    for k in range(FC.N_PAIRS):
        cell = np.array([FC.cell_of(l, p) for p in range(PC.patches(l))])
        kind = np.array([s.kinds[k][c][0] for c in cell])
        ident, const = kind == "identical", kind == "constant"
        assert ident.any() == (k == 1) and const.any() == (k == 2)
        assert not applied[k][ident].any() and _same_bits(got[k][ident], plain[k][ident]) and _same_bits(quality[k][ident], plain_q[k][ident])
        assert np.abs(got[k][ident]).max(initial=0.0) <= T.TOL
        # (of the predictions: at a frame corner the clamp may leave (0, 0) of any prediction, and applied is held to the clamp above)
        assert pred[k][~ident].all(axis=-1).all() and applied[k][~ident].any(axis=-1).sum() >= (~ident).sum() - 4
        # the constant cell (tests/test_fft_pred_field_host.py): the reference's long-range shift of a flat surface is finite,
        # (1 - N / 2, 1 - N / 2), so the cell predicts (-60, -60); every window pair with a constant current window answers alike, and the
        # total is the applied prediction plus that -- NaN where it passes max_px_speed
        if const.any():
            c = int(cell[const][0])
            assert np.abs(coarse[k, c] + (l.n / 2 - 1)).max() <= T.TOL
            assert (pred[k][const] == (-60, -60)).all()
            want = PC.total_np(applied[k][const], np.full((int(const.sum()), 2), 1.0 - l.n / 2))
            assert np.array_equal(np.isnan(got[k][const]), np.isnan(want))
            assert np.abs(got[k][const] - want)[~np.isnan(want)].max(initial=0.0) <= T.TOL


# ---- C.6: the response gate on a mixed field ----
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_response_gate_on_a_mixed_field(gpu, name, route):
    """one cell's previous content is unrelated; armed between its long-range response and the others', exactly that cell predicts 0 and
    the others keep their predictions; the outputs are the composition on an engine armed alike"""
    g = FC.gate_case(name)
    l = g.layout
    fm, second = _engine(l, route, min_response=g.threshold), _engine(l, route, min_response=g.threshold)
    cur, prev = _frames(l, g.cur, gpu), _frames(l, g.prev, gpu)
    got, quality, applied, coarse = (_np(t) for t in fm.process_coarse_to_fine_batch_device(cur, prev, **C2F))
    # the long-range pass, armed: the gated cell is NaN, the others have the unarmed entry's bits; the threshold (the oracle's) parts the
    # device's responses as it parts the oracle's
    lr, lr_q = (_np(t) for t in _engine(l, route).process_long_range_batch_device(cur, prev, return_quality=True))
    keep = np.arange(coarse.shape[1]) != FC.GATE_CELL
    assert lr_q[0, FC.GATE_CELL, 0] < g.threshold < lr_q[0, keep, 0].min(), (lr_q[0, :, 0], g.responses)
    assert np.isnan(coarse[0, FC.GATE_CELL]).all() and _same_bits(coarse[0, keep], lr[0, keep]) and not np.isnan(lr).any()
    gated64 = g.coarse64.copy()
    gated64[0, FC.GATE_CELL] = np.nan
    pred = PC.c2f_pred_np(l, coarse)
    assert np.array_equal(pred, PC.c2f_pred_np(l, gated64))
    assert np.array_equal(applied, PC.applied_np(l, pred))
    mine = np.array([FC.cell_of(l, p) == FC.GATE_CELL for p in range(PC.patches(l))])
    assert mine.any() and not pred[0][mine].any() and not applied[0][mine].any()
    assert pred[0][~mine].all(axis=-1).all() and applied[0][~mine].any(axis=-1).sum() >= (~mine).sum() - 4  # (a frame corner may clamp to (0, 0))
    _composition(second, cur, prev, pred, got, quality, applied, gpu)
    # (the gate acts on the fine pass too: a shift whose own response is under the threshold is NaN)
    assert np.isnan(got[0][~(quality[0, :, 0] >= g.threshold)]).all()
    assert not np.isnan(got[0][~mine]).all()


# ---- C.7: the stateful entry ----
@pytest.mark.parametrize("route", ROUTES)
def test_stateful_entry_on_a_field(gpu, route):
    s = FC.scene("f_8x12")
    l = s.layout
    fm, batch = _engine(l, route), _engine(l, route)
    want, want_q = (_np(t)[0] for t in batch.process_coarse_to_fine_batch_device(_frames(l, s.cur[:1], gpu), _frames(l, s.prev[:1], gpu), return_quality=True))
    first = fm.process_image_coarse_to_fine(s.prev[0])
    assert np.abs(first).max() <= T.TOL and fm.last_invalid == 0
    got = fm.process_image_coarse_to_fine(s.cur[0])
    assert _same_bits(got, want) and _same_bits(fm.last_quality, want_q)
    assert fm.last_invalid == int(np.isnan(want[:, 0]).sum())


# ---- D: coarse to fine on every pair route ----
@pytest.mark.parametrize("n", FC.ROUTE_SIZES)
def test_coarse_to_fine_on_every_pair_route(gpu, n):
    """a 4 x 4 grid of n x n patches under a planted (24, -20): the long-range pass runs the full-tile kernels of the family while the
    fine pass runs the engine's own route, both on the engine's scratch, quality buffer and fence. The kernel and whether a fused form
    exists come from the recorded route table, not from the engine."""
    r = FC.route_case(n)
    l = r.layout
    fused = FC.route_fused(n)
    cur, prev = _frames(l, r.cur, gpu), _frames(l, r.prev, gpu)
    outs = {}
    for route in ROUTES if fused else ROUTES[:1]:
        fm, second = _engine(l, route), _engine(l, route)
        assert fm.pred_route_supported("fused") == fused
        label = f"pred_route/n{n}/{route}"
        got, quality, applied, coarse, pred = _coarse_and_map(fm, l, cur, prev, r.cur, r.prev, r.coarse64, r.coarse32, label)
        _composition(second, cur, prev, pred, got, quality, applied, gpu)
        free = (applied == pred).all(axis=-1)
        assert np.array_equal(free, r.free) and ((~free).sum(axis=1) == FC.route_clamped(n)).all()
        worst, left_out = 0.0, 0
        for k in range(FC.ROUTE_PAIRS):
            for p in range(PC.patches(l)):
                if not r.clear[k, p]:
                    assert not free[k, p], ("a patch whose clamp is inactive must have a clear peak", k, p)
                    left_out += 1
                    continue
                res = got[k, p] - applied[k, p]
                worst = max(worst, float(np.abs(res - r.w64[k, p]).max()))
                assert T.check_patch(res, r.w64[k, p], r.w32[k, p], f"{label}/pair{k}", p, what="coarse to fine",
                                     pixels=(PC.window(l, r.cur[k], p), PC.window(l, r.disp[k], p))), (n, route, k, p)
        print(f"n={n} {l.variant} ({route}): worst |residual - f64 oracle| = {worst:.3g} px, {left_out} of {int((~free).sum())} clamped patches left out")
        outs[route] = (got, quality, applied, coarse)
    if fused:
        for a, b in zip(outs["fused"], outs["gather"]):
            assert _same_bits(a, b)
    else:
        assert not _engine(l, "gather").pred_route_supported("fused")
