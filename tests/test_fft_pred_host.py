"""No-GPU tests of the predicted-shift window offsets (include/mof.h, "Predicted-shift window offsets"): the two pure host helpers that
state the definitions, held to numpy (tests/pred_cases.py), the surfaces that must name the same entries, and -- on the CPU oracle -- the
facts the GPU tests rely on: the residuals of their inputs have clear peaks, and the coarse-to-fine ground is the one the feature adds."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import pred_cases as PC
import route_cases as R
import tolerances
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


@pytest.mark.parametrize("l", PC.LAYOUTS + PC.EDGE_LAYOUTS, ids=lambda l: l.name)
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


# sha256 (first 16 hex digits) of case(name).pred and .cur as they stood before the edge layouts scaled the recipe: the existing cases keep
# their exact bytes
CASE_BYTES = {
    "k1_32": ("8528097a29f49158", "79683bac60f40fb4"), "k1_64": ("6228ecabccfba0c3", "b75eafe2f626874a"),
    "n120": ("ef04cf11cbca1f7e", "00374b935aa6fd4a"), "persistent_128": ("ab34f257da4708c9", "4116cb084bd3ca53"),
    "k1h_96": ("8c2de2ebd1d127fd", "e5a06506d8a71efc"), "k1h_160": ("d62cc160b61fa154", "e81c59b917e38d79"),
    "planned_62": ("1dbb5dee0c059cb9", "e3728fd4188daa6f"), "large_200": ("b5f9de8fe845ce16", "63ff537882016641"),
    "offset_32": ("5bc8b7ac5704e1a2", "531de39f6c325703"),
}


def test_existing_cases_keep_their_bytes():
    assert set(CASE_BYTES) == {l.name for l in PC.LAYOUTS}
    for name, want in CASE_BYTES.items():
        c = PC.case(name)
        assert c.pred.dtype == np.int32 and c.cur.dtype == np.uint8
        assert (hashlib.sha256(c.pred.tobytes()).hexdigest()[:16], hashlib.sha256(c.cur.tobytes()).hexdigest()[:16]) == want, name


def test_edge_layouts_stand_at_the_sizes_the_kernels_branch_on():
    """the byte copy (n < 16), two overlapping 16-byte chunks per row (16 < n < 32), an odd tail column (odd n), the padded and odd
    half-tile sizes of the fused form, the large pipeline's odd tail; the variant and the fused form by the recorded route table"""
    assert [l.n for l in PC.EDGE_LAYOUTS] == [8, 15, 20, 31, 37, 57, 136, 162, 244]
    table = R.default_table()
    offset = 0
    for l in PC.EDGE_LAYOUTS:
        row = table[(R.PEAK_OPENCV, l.n)]
        assert R.variant(row) == l.variant, (l.name, row)
        assert (row[2] > 0) == (l.name in PC.EDGE_FUSED), (l.name, row)
        assert min(l.grid) >= 2 and l.pitch >= l.w
        x1, y1 = PC.origin_of(l, PC.patches(l) - 1)
        assert x1 + l.n <= l.w and y1 + l.n <= l.h and l.w - (x1 + l.n) <= 2 and l.h - (y1 + l.n) <= 1  # the smallest frames
        offset += l.origin == (1, 1) and min(l.stride) > l.n and l.pitch > l.w
    assert offset >= 2
    assert [table[(R.PEAK_OPENCV, n)][1] for n in (57, 136, 162, 244)] == [60, 144, 162, 250]  # the transform sizes: padded but for 162


@pytest.mark.parametrize("l", PC.EDGE_LAYOUTS, ids=lambda l: l.name)
def test_cpu_oracle_residuals_of_the_edge_cases(l):
    """What the GPU tests rely on at the edge sizes: from 15 on every patch has a clear peak and the two oracles lie within 2e-5 px; at 8,
    where the 5 x 5 window is most of the surface, at most a quarter of the patches lack a clear peak (left out of the oracle comparison,
    never of the bit identities) and the others lie within 2e-5 px. The planted shift is max(1, n // 8), the predictions spread
    max(1, n // 16) around it, and the clamp acts."""
    c = PC.case(l.name)
    w64, w32, clear = PC.residual_oracles(l.name)
    assert np.abs(c.planted).max() == max(1, l.n // 8)
    spread = max(1, l.n // 16)
    assert np.abs(c.pred[0] - c.planted[0]).max() <= spread  # (pair 0: seeded only)
    assert (c.applied != c.pred).any() and (c.applied[1] != c.pred[1]).any(axis=-1).sum() >= PC.patches(l) - 2
    unclear = int((~clear).sum())
    assert unclear <= PC.unclear_cap(l.name), (unclear, np.argwhere(~clear).tolist())
    assert PC.unclear_cap(l.name) == (3 if l.n == 8 else 0)
    dd = np.abs(w64 - w32).max(axis=-1)
    assert np.isfinite(w64[clear]).all() and dd[clear].max() <= tolerances.F32_LIMITED_FROM
    # the plain entry is valid on every patch of the frames and of the displaced frames (no |shift| > n / 2): the bit identities compare numbers
    lay = PC.oracle_layout(l)
    for k in range(PC.N_PAIRS):
        assert not np.isnan(O.fft_process(c.cur[k], c.prev[k], lay, 64)[0]).any() and not np.isnan(O.fft_process(c.cur[k], c.disp[k], lay, 64)[0]).any(), k
    want = c.planted[:, None, :] - c.applied  # (no closeness asserted: at these sizes the 5 x 5 centroid is biased by a pixel and more)
    print(f"{l.name}: {unclear} of {clear.size} patches without a clear peak (cap {PC.unclear_cap(l.name)}); oracle distance on the others, worst {dd[clear].max():.2e} px; "
          f"residuals up to {np.abs(want).max()} px")
