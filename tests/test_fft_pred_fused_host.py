"""No-GPU tests of the fused window-offset route (include/mof.h, MOF_PRED_ROUTE_FUSED): where the route exists, held to the recorded route
table; the overlapping-layout cases of tests/pred_fused_cases.py are ordinary inputs (the rule of test_route_cases_host.py), so that the
GPU tests' bars hide nothing and add nothing to the session's relaxed-patch budget; and the unrolled restatement is pred_cases' own
displaced frame said another way."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import conditioning
import pred_cases as PC
import pred_fused_cases as F
import route_cases as R
import tolerances
from mrs_optic_flow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATHER, FUSED = 0, 1  # MOF_PRED_ROUTE_GATHER, MOF_PRED_ROUTE_FUSED


def _supported(n, model, route):
    cfg = _capi.FftConfig(4 * n, 4 * n, n, 1, 1, 0, 0, n, n, 80.0, 0, model, 55)
    return _capi.load().mof_fft_pred_route_supported(C.byref(cfg), route)


def test_route_supported_follows_the_recorded_route_table():
    """gather: every size. fused: exactly 32, 64, 128 and the sizes whose default route is the half-tile kernel, under cv::phaseCorrelate's
    model; nothing under the OpenCL model."""
    table = R.default_table()
    fused = []
    for n in range(2, 1000):
        row = table[(R.PEAK_OPENCV, n)]
        want = int(row is not None and (n in (32, 64, 128) or R.variant(row) == "planned-half"))
        assert _supported(n, R.PEAK_OPENCV, FUSED) == want, (n, row)
        assert _supported(n, R.PEAK_OPENCV, GATHER) == 1 and _supported(n, R.PEAK_OCL, GATHER) == 1
        assert _supported(n, R.PEAK_OCL, FUSED) == 0, n
        if want:
            fused.append(n)
    assert {32, 64, 120, 128, 60, 96, 100, 140, 192} <= set(fused) and 62 not in fused and 200 not in fused
    print(f"fused form at {len(fused)} of 998 patch sizes: {fused[:12]} ... {fused[-3:]}")
    lib = _capi.load()
    cfg = _capi.FftConfig(256, 256, 64, 1, 1, 0, 0, 64, 64, 80.0, 0, 0, 55)
    for route in (-1, 2, 7):
        assert lib.mof_fft_pred_route_supported(C.byref(cfg), route) == _capi.MOF_ERR_BAD_ARG
    assert lib.mof_fft_pred_route_supported(None, FUSED) == _capi.MOF_ERR_BAD_ARG
    assert lib.mof_fft_set_pred_route(None, FUSED) == _capi.MOF_ERR_NOT_INIT and lib.mof_fft_pred_route(None) == GATHER


def test_companion_header_binding_and_cpp_forwarders_name_the_same_entries():
    """the route's entries live beside the pinned surface of include/mof.h: in include/mof_pred_route.h (which mof.h includes), the
    binding's PRED_ROUTE_SYMBOLS and the forwarders of include/mof/pred_route.hpp -- the same four everywhere, all exported"""
    entries = {"mof_fft_set_pred_route", "mof_fft_pred_route", "mof_fft_pred_route_supported", "mof_fft_process_batch_device_pred_bgr"}
    header = open(os.path.join(ROOT, "include", "mof_pred_route.h")).read()
    assert set(re.findall(r"^int (mof_\w+)\(", header, re.M)) == entries
    assert re.search(r"^#define MOF_PRED_ROUTE_GATHER 0$", header, re.M) and re.search(r"^#define MOF_PRED_ROUTE_FUSED 1$", header, re.M)
    assert '#include "mof_pred_route.h"' in open(os.path.join(ROOT, "include", "mof.h")).read()
    assert set(_capi.PRED_ROUTE_SYMBOLS) == entries and not entries & set(_capi.SYMBOLS)
    lib = _capi.load()
    for name in entries:
        assert getattr(lib, name).argtypes is not None, name
    forwarders = open(os.path.join(ROOT, "include", "mof", "pred_route.hpp")).read()
    assert set(re.findall(r"\b(mof_fft_\w+)\(", forwarders)) == entries - {"mof_fft_pred_route_supported"}  # (a plain C call, as the other pure helpers)
    hpp = open(os.path.join(ROOT, "include", "mof", "processors.hpp")).read()
    for method in ("setPredRoute", "predRoute", "processBatchDevicePredBgr"):
        assert re.search(r"\b%s\(" % method, hpp), method
    from mrs_optic_flow_amd import FftMethod

    for method in ("set_pred_route", "pred_route_supported", "process_batch_device_pred_bgr"):
        assert callable(getattr(FftMethod, method)), method
    assert isinstance(FftMethod.pred_route, property)


def test_overlapping_layouts_overlap_and_fit_their_frames():
    for l in F.OVER:
        assert l.stride[0] < l.n or l.stride[1] < l.n, l.name
        assert min(l.grid) >= 2 and l.pitch >= l.w
        x1, y1 = PC.origin_of(l, PC.patches(l) - 1)
        assert x1 + l.n <= l.w and y1 + l.n <= l.h, l.name
        assert _supported(l.n, R.PEAK_OPENCV, FUSED) == 1


@pytest.mark.parametrize("l", F.OVER, ids=lambda l: l.name)
def test_case_is_pinned_by_its_inputs(l):
    c = F.case(l.name)
    assert np.array_equal(c.applied, PC.applied_np(l, c.pred))
    assert (c.applied != c.pred).any(), "the clamp acts somewhere"
    assert np.abs(c.planted).max() <= l.n // 8
    w64, w32, clear = F.residual_oracles(l.name)
    assert clear.all(), np.argwhere(~clear).tolist()
    dd = np.abs(w64 - w32).max(axis=-1)
    print(f"{l.name}: oracle distance, worst {dd.max():.2e} px; residuals up to {np.abs(w64).max():.2f} px")
    assert np.isfinite(w64).all() and np.isfinite(w32).all()
    assert dd.max() <= tolerances.F32_LIMITED_FROM, dd
    lu = c.unrolled
    for k in range(F.N_PAIRS):
        for p in range(PC.patches(lu)):
            info = conditioning.analyse(PC.window(lu, c.cur_u[k], p), PC.window(lu, c.prev_u[k], p))
            allow, unpinned = tolerances.allowance(info, float(dd[k, p]))
            assert not unpinned and info["zero_bins"] == 0 and info["cancellation"] <= conditioning.CANCEL_FROM, (k, p, info)
            assert info["spread_px"] <= tolerances.F32_LIMITED_FROM and allow <= tolerances.SPREAD_FACTOR * tolerances.F32_LIMITED_FROM, (k, p, info, allow)


@pytest.mark.parametrize("name", ["k1_32", "offset_32", "n120"])
def test_unrolled_restatement_is_the_displaced_frame_patch_by_patch(name):
    """on a layout without overlap both restatements exist: patch q of prev' is the window q of pred_cases.displaced_np, patch q of cur'
    the window q of cur"""
    c = PC.case(name)
    l = c.layout
    lu = F.unrolled_layout(l)
    cu, pu = F.unroll_np(l, c.cur, c.prev, c.applied)
    assert cu.shape == (PC.N_PAIRS, l.grid[1] * l.n, l.grid[0] * l.n)
    for k in range(PC.N_PAIRS):
        for p in range(PC.patches(l)):
            assert np.array_equal(PC.window(lu, pu[k], p), PC.window(l, c.disp[k], p)), (k, p)
            assert np.array_equal(PC.window(lu, cu[k], p), PC.window(l, c.cur[k], p)), (k, p)


def test_bgr_frames_differ_per_channel_and_convert_as_the_kernels_do():
    c = F.case("over_32")
    bgr = F.bgr_of(c.cur)
    assert bgr.shape == c.cur.shape + (3,) and bgr.dtype == np.uint8
    assert (bgr[..., 0] != bgr[..., 1]).any() and (bgr[..., 1] != bgr[..., 2]).any() and (bgr[..., 0] != bgr[..., 2]).any()
    gray = F.gray_of_bgr(bgr)
    f = bgr.astype(np.float64)
    assert np.abs(gray - (0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2])).max() <= 0.51  # (CV_RGB2GRAY's weights, 14-bit fixed point)
