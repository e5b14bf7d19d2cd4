"""Inputs and numpy restatements for the tests of the FFT engine's predicted-shift window offsets (include/mof.h, "Predicted-shift
window offsets"): test_fft_pred_host.py (no GPU), test_gpu_fft_pred.py, test_gpu_cpp_pred.py. Nothing here touches a GPU.

The restatements are the header's definitions word for word: clamp_np (applied prediction), round4_np (prediction from a long-range
shift), displaced_np (the previous frame whose patch windows were read at the applied prediction) and total_np (applied + residual,
the speed gate on the total)."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
from mrs_optic_flow_amd import synth

I32_MIN, I32_MAX = -2**31, 2**31 - 1
SPEED = 80.0

# One layout per pair route of the engine (csrc/mof_capi.hip, fft_route), the smallest frames with more than one patch per axis, plus one
# that has origin (1, 1), stride > patch, a non-square frame and pitch > width. variant: what mof_fft_kernel_variant names.
Layout = namedtuple("Layout", "name n w h grid origin stride pitch variant")
LAYOUTS = [
    Layout("k1_32", 32, 128, 128, (4, 4), (0, 0), (32, 32), 128, "stockham"),
    Layout("k1_64", 64, 192, 128, (3, 2), (0, 0), (64, 64), 192, "stockham"),
    Layout("n120", 120, 240, 240, (2, 2), (0, 0), (120, 120), 240, "planned-half"),  # (the tuned size the half-tile kernel serves by default)
    Layout("persistent_128", 128, 256, 256, (2, 2), (0, 0), (128, 128), 256, "stockham"),
    Layout("k1h_96", 96, 192, 192, (2, 2), (0, 0), (96, 96), 192, "planned-half"),
    Layout("k1h_160", 160, 320, 320, (2, 2), (0, 0), (160, 160), 320, "planned-half"),
    Layout("planned_62", 62, 130, 126, (2, 2), (1, 1), (65, 63), 130, "planned"),
    Layout("large_200", 200, 400, 400, (2, 2), (0, 0), (200, 200), 400, "planned-large"),
    Layout("offset_32", 32, 150, 110, (4, 3), (1, 1), (36, 35), 160, "stockham"),
]
# The sizes the window-offset kernels branch on (csrc/pc_offset_kernel.hip: the byte copy under 16, the two overlapping 16-byte chunks
# of 16 < n < 32, a tail chunk at an odd column) and the padded and odd half-tile sizes of the fused form (57 -> 60, 136 -> 144, 162),
# plus a padded planned size and the large pipeline's odd tail. Three patches per row where that is cheap (an interior column, whose
# prediction the clamp leaves alone); four of them with origin (1, 1), stride > n and pitch > width. Their cases scale the recipe of
# `case` to the patch (EDGE_BLUR, _spread).
EDGE_LAYOUTS = [
    Layout("e_8", 8, 31, 19, (3, 2), (1, 1), (11, 10), 48, "planned"),
    Layout("e_15", 15, 45, 30, (3, 2), (0, 0), (15, 15), 45, "planned"),
    Layout("e_20", 20, 66, 43, (3, 2), (1, 1), (22, 21), 80, "planned"),
    Layout("e_31", 31, 93, 62, (3, 2), (0, 0), (31, 31), 93, "planned"),
    Layout("e_37", 37, 120, 77, (3, 2), (1, 1), (40, 38), 128, "planned"),
    Layout("e_57", 57, 114, 114, (2, 2), (0, 0), (57, 57), 114, "planned-half"),
    Layout("e_136", 136, 272, 272, (2, 2), (0, 0), (136, 136), 272, "planned-half"),
    Layout("e_162", 162, 330, 326, (2, 2), (1, 1), (165, 163), 336, "planned-half"),
    Layout("e_244", 244, 488, 488, (2, 2), (0, 0), (244, 244), 488, "planned-large"),
]
EDGE_FUSED = ["e_57", "e_136", "e_162"]  # those of EDGE_LAYOUTS with a fused form (tests/golden/fft_route_table.txt: half_m > 0)
# the (1 6 1) blur has no spectral zero and keeps the two oracles within 2e-5 px of each other on every patch from 15 on; at 8 the box
# blur does (the mild one: 6.7e-5 px), at the price of patches without a clear peak -- at most unclear_cap of a case's patches. e_8's
# strides are the first (of 9 .. 11 per axis) under which the plain entry is valid on every patch of the frames and of the displaced
# frames (no |shift| > n / 2) on the f64 oracle; they leave every patch with a clear peak.
EDGE_BLUR = {l.name: ("mild" if l.n >= 15 else True) for l in EDGE_LAYOUTS}
BY_NAME = {l.name: l for l in LAYOUTS + EDGE_LAYOUTS}
N_PAIRS = 2


def unclear_cap(name):
    """how many patches of a case may lack a clear peak and be left out of the ORACLE comparison (never of the bit identities): a
    quarter at n = 8, where the 5 x 5 window is most of the surface; none anywhere else"""
    l = BY_NAME[name]
    return N_PAIRS * patches(l) // 4 if l.n == 8 else 0


def patches(l):
    return l.grid[0] * l.grid[1]


def origin_of(l, p):
    return l.origin[0] + (p % l.grid[0]) * l.stride[0], l.origin[1] + (p // l.grid[0]) * l.stride[1]


def oracle_layout(l, max_px_speed=SPEED):
    return O.fft_layout(l.w, l.h, l.n, l.grid[0], l.grid[1], l.origin, l.stride, max_px_speed)


def engine_kwargs(l):
    return dict(sample_point_size=l.n, max_px_speed=SPEED, frame_shape=(l.h, l.w), grid=l.grid, origin=l.origin, stride=l.stride)


def clamp_np(l, p, px, py):
    """a of patch p for prediction (px, py): min(max(p, x0 - (W - n)), x0) per axis, in Python integers"""
    x0, y0 = origin_of(l, p)
    return min(max(int(px), x0 - (l.w - l.n)), x0), min(max(int(py), y0 - (l.h - l.n)), y0)


def round4_np(sx, sy):
    """p of a long-range shift: rint(4 s) in fp64, half to even (np.rint); a NaN shift predicts (0, 0)"""
    if np.isnan(sx) or np.isnan(sy):
        return 0, 0
    return tuple(int(np.clip(np.rint(4.0 * np.float64(v)), I32_MIN, I32_MAX)) for v in (sx, sy))


def applied_np(l, pred):
    """[pairs, patches, 2] int64 applied predictions of the int predictions `pred`"""
    out = np.zeros(pred.shape, np.int64)
    for k in range(pred.shape[0]):
        for p in range(pred.shape[1]):
            out[k, p] = clamp_np(l, p, pred[k, p, 0], pred[k, p, 1])
    return out


def displaced_np(l, prev, applied):
    """prev [pairs, H, W] with every patch window replaced by the window at (x0 - a_x, y0 - a_y); zero elsewhere"""
    out = np.zeros_like(prev)
    for k in range(prev.shape[0]):
        for p in range(applied.shape[1]):
            x0, y0 = origin_of(l, p)
            ax, ay = (int(v) for v in applied[k, p])
            out[k, y0:y0 + l.n, x0:x0 + l.n] = prev[k, y0 - ay:y0 - ay + l.n, x0 - ax:x0 - ax + l.n]
    return out


def total_np(applied, residual, max_px_speed=SPEED):
    """d = a + r per component (a zero component keeps r's bits); (NaN, NaN) where r is NaN or |d|^2 > max_px_speed^2 -- a patch with
    a = (0, 0) is r itself"""
    a = applied.astype(np.float64)
    d = np.where(applied == 0, residual, a + residual)
    moved = (applied != 0).any(axis=-1)
    bad = np.isnan(residual).any(axis=-1) | (moved & (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] > max_px_speed * max_px_speed))
    d[bad] = np.nan
    return d


Case = namedtuple("Case", "layout cur prev planted pred applied disp")


def _planted(l, k):
    """a planted shift no larger than n / 8 on either axis (at least 1), different per pair"""
    m = max(1, l.n // 8)
    return (m if k % 2 == 0 else -(m - 1)), (-(m - 1) if k % 2 == 0 else m)


@functools.lru_cache(maxsize=None)
def case(name):
    """N_PAIRS pairs: seeded predictions per patch within +-3 of the pair's planted shift (EDGE_LAYOUTS: within +-max(1, n // 16), on
    their own blur); the last pair's border patches predict OUTWARDS instead -- +-n and the int32 extremes alternate -- so that the clamp
    acts on them (and leaves a small residual)."""
    l = BY_NAME[name]
    edge = name in EDGE_BLUR
    spread = max(1, l.n // 16) if edge else 3
    rng = np.random.RandomState(0x9ED0 + l.n + l.w)
    cur, prev, planted = [], [], []
    for k in range(N_PAIRS):
        dx, dy = _planted(l, k)
        c, p = synth.pair_np(40 + k, l.h, l.w, dx, dy, blur=EDGE_BLUR[name]) if edge else synth.pair_np(40 + k, l.h, l.w, dx, dy)
        cur.append(c)
        prev.append(p)
        planted.append((dx, dy))
    cur, prev, planted = np.stack(cur), np.stack(prev), np.array(planted)
    pred = planted[:, None, :] + rng.randint(-spread, spread + 1, size=(N_PAIRS, patches(l), 2))
    gx, gy = l.grid
    k = N_PAIRS - 1
    for p in range(patches(l)):
        i, j = p % gx, p // gx
        if i == 0:
            pred[k, p, 0] = I32_MAX if j % 2 == 0 else l.n
        elif i == gx - 1:
            pred[k, p, 0] = I32_MIN if j % 2 == 0 else -l.n
        if j == 0:
            pred[k, p, 1] = l.n if i % 2 == 0 else I32_MAX
        elif j == gy - 1:
            pred[k, p, 1] = -l.n if i % 2 == 0 else I32_MIN
    pred = pred.astype(np.int32)
    applied = applied_np(l, pred)
    disp = displaced_np(l, prev, applied)
    for a in (cur, prev, pred, applied, disp):
        a.setflags(write=False)
    return Case(l, cur, prev, planted, pred, applied, disp)


def window(l, frame, p):
    x0, y0 = origin_of(l, p)
    return frame[y0:y0 + l.n, x0:x0 + l.n]


@functools.lru_cache(maxsize=None)
def residual_oracles(name):
    """per pair and patch: -O.phase_correlate(cur window, displaced prev window) at 64 and 32 bit, and whether the f64 surface has a
    clear peak (second-highest value outside the 5 x 5 window < half the peak)"""
    c = case(name)
    l = c.layout
    w64 = np.zeros((N_PAIRS, patches(l), 2))
    w32 = np.zeros_like(w64)
    clear = np.zeros((N_PAIRS, patches(l)), bool)
    for k in range(N_PAIRS):
        for p in range(patches(l)):
            a, b = window(l, c.cur[k], p), window(l, c.disp[k], p)
            (x, y), d = O.phase_correlate(a, b, 64)
            w64[k, p] = (-x, -y)
            clear[k, p] = d["second_value"] < 0.5 * d["peak_value"]
            (x, y), _ = O.phase_correlate(a, b, 32)
            w32[k, p] = (-x, -y)
    return w64, w32, clear


# ---- coarse to fine: N = 32 on the reference tiling, a planted shift beyond N / 2 (pair 0) and an identical pair (pair 1) ----
C2F = {128: (24, -20), 160: (-22, 19)}
C2F_MAX_LEFT_OUT = {128: (7, 3), 160: (9, 2)}  # frame -> (clamped patches, how many of them may lack a clear peak)


def c2f_layout(fs):
    g = fs // 32
    return Layout(f"c2f_{fs}", 32, fs, fs, (g, g), (0, 0), (32, 32), fs, "stockham")


@functools.lru_cache(maxsize=None)
def c2f_case(fs):
    l = c2f_layout(fs)
    dx, dy = C2F[fs]
    c0, p0 = synth.pair_np(3, fs, fs, dx, dy)
    c1, p1 = synth.pair_np(5, fs, fs, 0, 0, kind="identical")
    cur, prev = np.stack([c0, c1]), np.stack([p0, p1])
    lay = oracle_layout(l)
    coarse64 = np.stack([O.fft_process_long_range(cur[k], prev[k], lay, 64)[0] for k in range(2)])
    coarse32 = np.stack([O.fft_process_long_range(cur[k], prev[k], lay, 32)[0] for k in range(2)])
    return l, cur, prev, coarse64, coarse32


def c2f_pred_np(l, coarse):
    """[pairs, patches, 2] predictions from [pairs, lr patches, 2] long-range shifts"""
    gx, gy = l.grid
    gxl, gyl = gx // 4, gy // 4
    pred = np.zeros((coarse.shape[0], gx * gy, 2), np.int64)
    for k in range(coarse.shape[0]):
        for p in range(gx * gy):
            li, lj = min((p % gx) // 4, gxl - 1), min((p // gx) // 4, gyl - 1)
            pred[k, p] = round4_np(*coarse[k, lj * gxl + li])
    return pred
