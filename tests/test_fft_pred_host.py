"""No-GPU tests of the predicted-shift window offsets (include/mof.h, "Predicted-shift window offsets"): the two pure host helpers that
state the definitions, held to numpy (tests/pred_cases.py), the surfaces that must name the same entries, and -- on the CPU oracle -- the
facts the GPU tests rely on: the residuals of their inputs have clear peaks, and the coarse-to-fine ground is the one the feature adds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pred_cases as PC
from mrs_optic_flow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD = _capi.MOF_OK, _capi.MOF_ERR_BAD_ARG
I32_MIN, I32_MAX = PC.I32_MIN, PC.I32_MAX


def _cfg(l):
    return _capi.FftConfig(l.w, l.h, l.n, l.grid[0], l.grid[1], l.origin[0], l.origin[1], l.stride[0], l.stride[1], PC.SPEED, 0, 0, 55)


def _clamp(cfg, patch, px, py):
    ax, ay = C.c_int32(-7), C.c_int32(-7)
    rc = _capi.load().mof_fft_pred_clamp(C.byref(cfg), patch, px, py, C.byref(ax), C.byref(ay))
    return rc, (ax.value, ay.value)


def _from_coarse(sx, sy):
    px, py = C.c_int32(-7), C.c_int32(-7)
    rc = _capi.load().mof_fft_pred_from_coarse(sx, sy, C.byref(px), C.byref(py))
    return rc, (px.value, py.value)


@pytest.mark.parametrize("l", PC.LAYOUTS, ids=lambda l: l.name)
def test_clamp_matches_numpy_on_every_border_case(l):
    """every patch of the layout x predictions at, one inside and one outside each clamp bound, 0, +-n and the int32 extremes"""
    cfg = _cfg(l)
    for p in range(PC.patches(l)):
        x0, y0 = PC.origin_of(l, p)
        xs = sorted({0, l.n, -l.n, I32_MIN, I32_MAX, I32_MIN + 1, I32_MAX - 1} | {b + d for b in (x0, x0 - (l.w - l.n)) for d in (-1, 0, 1)})
        ys = sorted({0, l.n, -l.n, I32_MIN, I32_MAX} | {b + d for b in (y0, y0 - (l.h - l.n)) for d in (-1, 0, 1)})
        for i, px in enumerate(xs):
            py = ys[i % len(ys)]
            assert _clamp(cfg, p, px, py) == (OK, PC.clamp_np(l, p, px, py)), (p, px, py)
        for i, py in enumerate(ys):
            px = xs[i % len(xs)]
            assert _clamp(cfg, p, px, py) == (OK, PC.clamp_np(l, p, px, py)), (p, px, py)
        ax, ay = _clamp(cfg, p, I32_MIN, I32_MAX)[1]
        assert 0 <= x0 - ax <= l.w - l.n and 0 <= y0 - ay <= l.h - l.n  # the window stays inside the frame


def test_clamp_patch_as_large_as_the_frame():
    """n == W: the only applied prediction is 0, whatever is predicted"""
    l = PC.Layout("whole", 64, 64, 96, (1, 1), (0, 0), (64, 64), 64, "stockham")
    cfg = _cfg(l)
    for px in (I32_MIN, -64, -1, 0, 1, 64, I32_MAX):
        for py in (I32_MIN, -33, -32, 0, 1, I32_MAX):
            rc, (ax, ay) = _clamp(cfg, 0, px, py)
            assert rc == OK and ax == 0 and (ax, ay) == PC.clamp_np(l, 0, px, py), (px, py)
            assert -32 <= ay <= 0


def test_clamp_argument_checks():
    l = PC.BY_NAME["k1_32"]
    cfg = _cfg(l)
    lib = _capi.load()
    a = C.c_int32(0)
    assert _clamp(cfg, -1, 0, 0)[0] == BAD and _clamp(cfg, PC.patches(l), 0, 0)[0] == BAD
    assert lib.mof_fft_pred_clamp(None, 0, 0, 0, C.byref(a), C.byref(a)) == BAD
    assert lib.mof_fft_pred_clamp(C.byref(cfg), 0, 0, 0, None, C.byref(a)) == BAD
    assert lib.mof_fft_pred_clamp(C.byref(cfg), 0, 0, 0, C.byref(a), None) == BAD
    bad = _cfg(l)
    bad.frame_width = 100  # the grid leaves the frame
    assert _clamp(bad, 3, 0, 0)[0] == BAD
    assert lib.mof_fft_pred_from_coarse(0.0, 0.0, None, C.byref(a)) == BAD


def test_from_coarse_rounds_half_to_even_and_maps_nan_to_zero():
    nan, inf = float("nan"), float("inf")
    values = [0.0, -0.0, 0.125, -0.125, 0.375, -0.375, 0.625, 0.875, 1.125, 6.03, -4.80, 6.125, 6.375, -4.875, -4.625, 0.12499999999999999,
              0.12500000000000003, 5.999999, 1e-300, -1e-300, 2.0 ** 29 - 0.125, -(2.0 ** 29) - 0.125, 1e12, -1e12, inf, -inf]
    for sx in values:
        for sy in (values[(values.index(sx) + 5) % len(values)], 0.375, -0.625):
            assert _from_coarse(sx, sy) == (OK, PC.round4_np(sx, sy)), (sx, sy)
    # ties: 4 s = x.5 goes to the even neighbour
    assert _from_coarse(0.125, -0.125) == (OK, (0, 0)) and _from_coarse(0.375, -0.375) == (OK, (2, -2))
    assert _from_coarse(0.625, 0.875) == (OK, (2, 4)) and _from_coarse(-4.625, 6.125) == (OK, (-18, 24))
    assert _from_coarse(6.03, -4.80) == (OK, (24, -19))
    # NaN on either axis: (0, 0)
    for sx, sy in ((nan, 1.0), (1.0, nan), (nan, nan), (nan, inf)):
        assert _from_coarse(sx, sy) == (OK, (0, 0))
    assert _from_coarse(inf, -inf) == (OK, (I32_MAX, I32_MIN))


def test_header_binding_and_cpp_mirror_name_the_same_entries():
    entries = ["mof_fft_pred_clamp", "mof_fft_pred_from_coarse", "mof_fft_reserve_pred", "mof_fft_process_batch_device_pred",
               "mof_fft_process_coarse_to_fine_batch_device", "mof_fft_process_coarse_to_fine"]
    header = open(os.path.join(ROOT, "include", "mof.h")).read()
    declared = set(re.findall(r"^int (mof_fft_\w*(?:pred|coarse)\w*)\(", header, re.M))
    assert declared == set(entries)
    bound = {s for s in _capi.SYMBOLS if re.search(r"mof_fft_\w*(pred|coarse)", s)}
    assert bound == set(entries)
    lib = _capi.load()
    for name in entries:
        assert getattr(lib, name) is not None
    hpp = open(os.path.join(ROOT, "include", "mof", "processors.hpp")).read()
    called = set(re.findall(r"\b(mof_fft_\w*(?:pred|coarse)\w*)\(", hpp))
    assert called == set(entries) - {"mof_fft_pred_clamp", "mof_fft_pred_from_coarse"}  # (the helpers are plain C calls)
    for method in ("processBatchDevicePred", "processCoarseToFineBatchDevice", "processImageCoarseToFine", "reservePred"):
        assert re.search(r"\b%s\(" % method, hpp), method
    from mrs_optic_flow_amd import FftMethod

    for method in ("process_batch_device_pred", "process_coarse_to_fine_batch_device", "process_image_coarse_to_fine", "reserve_pred"):
        assert callable(getattr(FftMethod, method)), method


@pytest.mark.parametrize("l", PC.LAYOUTS, ids=lambda l: l.name)
def test_cpu_oracle_residuals_of_the_gpu_inputs_are_small_and_clear(l):
    """What test_gpu_fft_pred.py's oracle test relies on: on its inputs every residual is a small shift with a clear peak, equal to
    planted - applied, and the two oracles agree within the fast path of tests/tolerances.py on (nearly) every patch."""
    c = PC.case(l.name)
    w64, w32, clear = PC.residual_oracles(l.name)
    assert clear.all()
    want = c.planted[:, None, :] - c.applied
    assert np.abs(want).max() < l.n // 2 - 4  # well inside what a patch can measure (offset_32: 11, its frame has room past the grid)
    # (the 5 x 5 centroid of a non-periodic shift is biased towards 0 by the uncorrelated border, up to half a pixel at n = 32: the
    # integer peak is the planted residual)
    assert np.abs(w64 - want).max() < 1.0 and np.abs(w32 - want).max() < 1.0
    # the extremes at the borders were clamped, the seeded interior was not
    assert (c.applied != c.pred).any() and ((c.applied == c.pred).all(axis=-1).any() or min(l.grid) < 3)
    print(l.name, "oracle-to-oracle distance, worst:", float(np.abs(w64 - w32).max()))


@pytest.mark.parametrize("fs", sorted(PC.C2F))
def test_cpu_oracle_coarse_to_fine_ground(fs):
    """The issue's table on the CPU oracle: the plain field is wrong on at least half the patches; the long-range oracle's prediction is
    safely off a rounding tie; with the offset windows every patch whose clamp is inactive has a clear peak and lands within 0.25 px of
    the planted shift; of the clamped patches at most the stated number lack a clear peak."""
    l, cur, prev, coarse64, coarse32 = PC.c2f_case(fs)
    planted = np.array(PC.C2F[fs])
    lay = PC.oracle_layout(l)
    plain, _ = O.fft_process(cur[0], prev[0], lay, 64)
    wrong = ~(np.abs(plain - planted).max(axis=-1) <= 0.5)
    assert wrong.sum() * 2 >= PC.patches(l), wrong.sum()
    tie = np.abs(4.0 * coarse64[0] - np.floor(4.0 * coarse64[0]) - 0.5)
    assert tie.min() > 0.1 and np.array_equal(PC.c2f_pred_np(l, coarse64), PC.c2f_pred_np(l, coarse32))
    pred = PC.c2f_pred_np(l, coarse64)
    assert (pred[1] == 0).all()  # the identical pair
    applied = PC.applied_np(l, pred)
    disp = PC.displaced_np(l, prev, applied)
    free = (applied[0] == pred[0]).all(axis=-1)
    n_clamped, may_skip = PC.C2F_MAX_LEFT_OUT[fs]
    assert (~free).sum() == n_clamped
    skipped, worst = 0, 0.0
    for p in range(PC.patches(l)):
        (x, y), d = O.phase_correlate(PC.window(l, cur[0], p), PC.window(l, disp[0], p), 64)
        clear = d["second_value"] < 0.5 * d["peak_value"]
        if free[p]:
            assert clear, p
            total = applied[0, p] + np.array([-x, -y])
            worst = max(worst, float(np.abs(total - planted).max()))
        else:
            skipped += not clear
    assert worst <= 0.25 and skipped <= may_skip, (worst, skipped)
    print(f"frame {fs}: plain wrong on {int(wrong.sum())} of {PC.patches(l)}, prediction {pred[0, 0].tolist()}, worst free patch {worst:.3f} px, "
          f"{skipped} of {n_clamped} clamped patches without a clear peak")
