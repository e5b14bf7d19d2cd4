"""Inputs and numpy restatements for the tests of the FFT engine's FUSED window-offset route (include/mof.h, MOF_PRED_ROUTE_FUSED):
test_fft_pred_fused_host.py (no GPU), test_gpu_fft_pred_fused.py, test_gpu_cpp_pred_fused.py. Built on tests/pred_cases.py; nothing here
touches a GPU.

The ground the fused route adds is the layout whose patches OVERLAP (the gather cannot serve it: overlapping windows cannot share one
displaced frame). One such layout per kernel path, the smallest with more than one patch per axis. The reference for them is the
"unrolled" restatement: for a layout L the non-overlapping layout L' with the same patch size and grid, stride = patch size, origin 0;
patch q of cur' is the window of cur at q, patch q of prev' the window of prev at (x0 - a_x, y0 - a_y). The kernels' arithmetic depends
on the pixels of the two windows, not on where they lie, so the plain entry of an engine of layout L' on (cur', prev') gives the
residuals bit for bit."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
import pred_cases as PC
from mrs_optic_flow_amd import synth

Layout = PC.Layout
# name, n, frame w x h, grid, origin, stride, pitch, variant; in the comments the kernel path
OVER = [
    Layout("over_32", 32, 128, 128, (4, 4), (0, 0), (24, 24), 128, "stockham"),        # K1
    Layout("over_64", 64, 200, 150, (3, 2), (1, 1), (60, 50), 208, "stockham"),        # K1
    Layout("over_128", 128, 320, 224, (3, 2), (0, 0), (96, 96), 320, "stockham"),      # K1, the persistent loop
    Layout("over_120", 120, 300, 240, (3, 2), (0, 0), (90, 100), 300, "planned-half"),  # K1h, the general loader
    Layout("over_96", 96, 240, 192, (3, 2), (0, 0), (72, 96), 240, "planned-half"),    # K1h, the `fills` loader
    Layout("over_140", 140, 330, 300, (2, 2), (0, 0), (100, 130), 336, "planned-half"),  # K1h, padded to 144
]
BY_NAME = {l.name: l for l in OVER}
N_PAIRS = PC.N_PAIRS
# The texture index of pair k of a case is SEEDS[name] + k. Chosen on the CPU, from the oracles and the pixels alone, so that
# test_fft_pred_fused_host.py holds on every patch (the two oracles within tolerances.F32_LIMITED_FROM, no relaxing mechanism, a clear
# peak): the first index from 40 on -- pred_cases.case's own -- for which it does. The GPU tests then meet no patch off the fast path.
SEEDS = {"over_32": 40, "over_64": 40, "over_128": 40, "over_120": 40, "over_96": 40, "over_140": 40}

Case = namedtuple("Case", "layout cur prev planted pred applied unrolled cur_u prev_u")


def unrolled_layout(l):
    """L': the same patch size and grid, stride = patch size, origin 0, a dense frame that the grid fills"""
    return Layout(l.name + "_unrolled", l.n, l.grid[0] * l.n, l.grid[1] * l.n, l.grid, (0, 0), (l.n, l.n), l.grid[0] * l.n, l.variant)


def unroll_np(l, cur, prev, applied):
    """(cur', prev') [pairs, gy n, gx n]: patch q of cur' = the window of cur at q, of prev' = the window of prev at (x0 - a_x, y0 - a_y)"""
    lu = unrolled_layout(l)
    cu = np.zeros((cur.shape[0], lu.h, lu.w), np.uint8)
    pu = np.zeros_like(cu)
    for k in range(cur.shape[0]):
        for p in range(PC.patches(l)):
            x0, y0 = PC.origin_of(l, p)
            u0, v0 = PC.origin_of(lu, p)
            ax, ay = (int(v) for v in applied[k, p])
            cu[k, v0:v0 + l.n, u0:u0 + l.n] = cur[k, y0:y0 + l.n, x0:x0 + l.n]
            pu[k, v0:v0 + l.n, u0:u0 + l.n] = prev[k, y0 - ay:y0 - ay + l.n, x0 - ax:x0 - ax + l.n]
    return cu, pu


def build(l, k0):
    """pred_cases.case's recipe on layout l with texture indices k0, k0 + 1: planted shifts of at most n / 8, predictions within +-3 of
    them, the last pair's border patches predicting outwards (+-n and the int32 extremes) so that the clamp acts"""
    rng = np.random.RandomState(0x9ED0 + l.n + l.w)
    cur, prev, planted = [], [], []
    for k in range(N_PAIRS):
        dx, dy = PC._planted(l, k)
        c, p = synth.pair_np(k0 + k, l.h, l.w, dx, dy)
        cur.append(c)
        prev.append(p)
        planted.append((dx, dy))
    cur, prev, planted = np.stack(cur), np.stack(prev), np.array(planted)
    pred = planted[:, None, :] + rng.randint(-3, 4, size=(N_PAIRS, PC.patches(l), 2))
    gx, gy = l.grid
    k = N_PAIRS - 1
    seeded = pred[k].copy()
    for p in range(PC.patches(l)):
        i, j = p % gx, p // gx
        if i == 0:
            pred[k, p, 0] = PC.I32_MAX if j % 2 == 0 else l.n
        elif i == gx - 1:
            pred[k, p, 0] = PC.I32_MIN if j % 2 == 0 else -l.n
        if j == 0:
            pred[k, p, 1] = l.n if i % 2 == 0 else PC.I32_MAX
        elif j == gy - 1:
            pred[k, p, 1] = -l.n if i % 2 == 0 else PC.I32_MIN
        # These frames have room past the grid (over_32: 24 px, a stride), so the clamp of an outward prediction at the far border can leave
        # a residual no patch of this size measures (over_32: 21 and 28 px at n = 32 -- no clear peak under any texture). Such a component
        # keeps its seeded prediction: the bound is test_fft_pred_host.py's, |planted - applied| < n / 2 - 4. The clamp still acts at every
        # near border (a = x0 = 0) and at the far borders with less room.
        a = PC.clamp_np(l, p, pred[k, p, 0], pred[k, p, 1])
        for ax in (0, 1):
            if abs(int(planted[k, ax]) - a[ax]) >= l.n // 2 - 4:
                pred[k, p, ax] = seeded[p, ax]
    pred = pred.astype(np.int32)
    applied = PC.applied_np(l, pred)
    cu, pu = unroll_np(l, cur, prev, applied)
    for a in (cur, prev, pred, applied, cu, pu):
        a.setflags(write=False)
    return Case(l, cur, prev, planted, pred, applied, unrolled_layout(l), cu, pu)


@functools.lru_cache(maxsize=None)
def case(name):
    return build(BY_NAME[name], SEEDS[name])


def oracles_of(c):
    """per pair and patch of a Case: -O.phase_correlate(cur' patch, prev' patch) at 64 and 32 bit, and whether the f64 surface has a clear
    peak (second value below half the peak)"""
    lu = c.unrolled
    w64 = np.zeros((N_PAIRS, PC.patches(lu), 2))
    w32 = np.zeros_like(w64)
    clear = np.zeros((N_PAIRS, PC.patches(lu)), bool)
    for k in range(N_PAIRS):
        for p in range(PC.patches(lu)):
            a, b = PC.window(lu, c.cur_u[k], p), PC.window(lu, c.prev_u[k], p)
            (x, y), d = O.phase_correlate(a, b, 64)
            w64[k, p] = (-x, -y)
            clear[k, p] = d["second_value"] < 0.5 * d["peak_value"]
            (x, y), _ = O.phase_correlate(a, b, 32)
            w32[k, p] = (-x, -y)
    return w64, w32, clear


@functools.lru_cache(maxsize=None)
def residual_oracles(name):
    return oracles_of(case(name))


def gray_of_bgr(frames):
    """CV_RGB2GRAY on interleaved BGR8 [..., 3] in the kernels' integer form: (c0 4899 + c1 9617 + c2 1868 + 8192) >> 14"""
    f = frames.astype(np.int64)
    return ((f[..., 0] * 4899 + f[..., 1] * 9617 + f[..., 2] * 1868 + 8192) >> 14).astype(np.uint8)


def bgr_of(frames):
    """interleaved BGR8 [n, H, W, 3] whose three channels differ, each a pointwise function of the gray frames (a planted shift stays
    one): f, (f + 85) mod 256, 255 - f"""
    return np.ascontiguousarray(np.stack([frames, frames + np.uint8(85), np.uint8(255) - frames], axis=-1))
