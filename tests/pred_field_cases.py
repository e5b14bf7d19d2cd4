"""Inputs for the tests that hold the coarse-to-fine PREDICTION MAP (csrc/pc_offset_kernel.hip, pc_pred_from_coarse_kernel) and coarse to
fine on every pair route: test_fft_pred_field_host.py (no GPU) and test_gpu_fft_pred_field.py. Built on tests/pred_cases.py, whose
restatements (c2f_pred_np, applied_np, displaced_np, total_np, round4_np) are the only ones; nothing here touches a GPU.

1. Piecewise shift fields (FIELDS). The map sends fine patch (i, j) of pair k to long-range patch (min(i / 4, gx_lr - 1),
   min(j / 4, gy_lr - 1)) of that pair. A long-range CELL is the 4N x 4N block of the frame one long-range patch sees; the last cell of a
   row or column also takes the ragged remainder of the frame. Every cell of every pair is cut on its own, from its own texture index,
   with its own planted integer shift (SHIFTS: multiples of 4 -- the quarter image of this texture decorrelates under any other shift --
   pairwise different inside a pair, at least one component beyond N / 2), and the assignment of shifts to cells rotates from pair to
   pair. In pair 1 one cell is an identical pair (prediction 0), in pair 2 one cell is constant in both frames (on the reference a flat
   surface answers (1 - N / 2, 1 - N / 2), finite: the cell predicts (-60, -60); the long-range patch that is NaN beside valid neighbours
   is the gate pair's, under an armed min_response). A transposed index, swapped i and j, a wrong divisor, a missing clamp of the ragged columns or a dropped pair offset
   each change the applied predictions (test_fft_pred_field_host.py shows that with numpy, on the oracle's long-range shifts).

   An INSIDE patch: its clamp is inactive (applied == prediction) and its displaced previous window lies wholly in its own cell, so both
   windows show one texture under one shift. Computed from the f64 oracle's long-range shifts and the geometry, never from an engine.
   Patches of the constant cell are never inside (no peak to hold).

   What test_fft_pred_field_host.py and test_gpu_fft_pred_field.py print for these scenes (N = 32; per pair: inside patches of the
   planted cells / patches of the planted cells; tie margin = worst |4 s - rint(4 s)| of a long-range component, bar 0.48; the residual
   column is the worst |residual - f64 oracle| of an inside patch on the device, gather = fused bit for bit):

       layout   grid     long-range   inside per pair            tie margin   worst residual - f64 oracle
       f_8x12   8 x 12   2 x 3        54/96   45/80   45/80      0.477        4.5e-07 px
       f_11x5   11 x 5   2 x 1        36/55   12/20   24/35      0.442        2.8e-07 px
       f_5x11   5 x 11   1 x 2        36/55   12/20   24/35      0.442        3.5e-07 px
       f_wide   8 x 4    2 x 1        21/32   9/16    9/16       0.442        1.9e-07 px

   (window offsets at n = 8, tests/pred_cases.py e_8: 0 of 12 patches lack a clear peak and are left out of the oracle comparison,
   cap 3.)

2. Coarse to fine on every pair route (ROUTE_SIZES): a 4 x 4 grid -- one long-range patch --, frame side 4 n, a uniform planted
   (24, -20), two pairs. 480 / 120 is the reference geometry."""
import functools
from collections import namedtuple

import numpy as np

import oracle_lib as O
import pred_cases as PC
import route_cases as R
from mrs_optic_flow_amd import synth

Layout = PC.Layout
N = 32
FIELDS = [
    Layout("f_8x12", N, 256, 384, (8, 12), (0, 0), (N, N), 256, "stockham"),  # the row stride of the coarse array: gx_lr != gy_lr, both > 1
    Layout("f_11x5", N, 352, 160, (11, 5), (0, 0), (N, N), 368, "stockham"),  # ragged columns 8 .. 10 and row 4 take the last cell
    Layout("f_5x11", N, 160, 352, (5, 11), (0, 0), (N, N), 160, "stockham"),  # the same, transposed
    Layout("f_wide", N, 300, 140, (8, 4), (0, 0), (N, N), 304, "stockham"),   # a frame larger than its tiling
]
BY_NAME = {l.name: l for l in FIELDS}
SHIFTS = [(24, -20), (-20, 24), (20, 28), (-24, -16), (16, -24), (-28, 20)]
N_PAIRS = 3
ROTATE = (0, 1, 3, 4)  # pair k's cell c is planted SHIFTS[(c + ROTATE[k]) % 6]; the last entry is the gate pair's
IDENTICAL = (1, -1)    # (pair, cell): the last cell of pair 1 is an identical pair
CONSTANT = (2, 0)      # the first cell of pair 2 is constant in both frames
# The texture index of cell c of pair k is SEEDS[name] + 8 k + c; of the gate pair GATE_SEEDS[name] + c (its unrelated previous content:
# + 64). Chosen on the CPU, from the oracles and the pixels alone: the first base from 40 on -- pred_cases.case's own -- for which
# test_fft_pred_field_host.py holds and every prediction of the f64 oracle lies within +-2 px of its planted shift.
SEEDS = {"f_8x12": 42, "f_11x5": 40, "f_5x11": 40, "f_wide": 40}
GATE_SEEDS = {"f_8x12": 42, "f_11x5": 40, "f_5x11": 40, "f_wide": 40}
GATE_CELL = 1          # the cell of the gate pair whose previous content is an unrelated texture


def lr_grid(l):
    return l.grid[0] // 4, l.grid[1] // 4


def cells(l):
    """[(x0, y0, x1, y1)] per long-range patch, in the order of the coarse array (lj * gx_lr + li)"""
    gxl, gyl = lr_grid(l)
    side = 4 * l.n
    return [(li * side, lj * side, l.w if li == gxl - 1 else (li + 1) * side, l.h if lj == gyl - 1 else (lj + 1) * side)
            for lj in range(gyl) for li in range(gxl)]


def cell_of(l, p):
    """the cell of fine patch p: the one that holds the patch's window (the map of include/mof.h, from the geometry)"""
    x0, y0 = PC.origin_of(l, p)
    hits = [c for c, (cx0, cy0, cx1, cy1) in enumerate(cells(l)) if cx0 <= x0 and x0 + l.n <= cx1 and cy0 <= y0 and y0 + l.n <= cy1]
    assert len(hits) == 1, (l.name, p, hits)
    return hits[0]


def kinds(l, k):
    """per cell of pair k: ("shift", dx, dy), ("identical", 0, 0) or ("constant", 0, 0)"""
    n = len(cells(l))
    out = []
    for c in range(n):
        if (k, c) in ((IDENTICAL[0], IDENTICAL[1] % n), (CONSTANT[0], CONSTANT[1] % n)):
            out.append(("identical" if k == IDENTICAL[0] else "constant", 0, 0))
        else:
            out.append(("shift",) + SHIFTS[(c + ROTATE[k]) % len(SHIFTS)])
    return out


def _paint(l, k, unrelated=None):
    cur, prev = np.zeros((l.h, l.w), np.uint8), np.zeros((l.h, l.w), np.uint8)
    for c, ((x0, y0, x1, y1), (kind, dx, dy)) in enumerate(zip(cells(l), kinds(l, k))):
        idx = GATE_SEEDS[l.name] + c if k == 3 else SEEDS[l.name] + 8 * k + c
        cc, pp = synth.pair_np(idx, y1 - y0, x1 - x0, dx, dy, kind=kind)
        if c == unrelated:
            pp = synth.pair_np(idx + 64, y1 - y0, x1 - x0, 0, 0)[1]
        cur[y0:y1, x0:x1], prev[y0:y1, x0:x1] = cc, pp
    return cur, prev


def _coarse(l, cur, prev, precision):
    lay = PC.oracle_layout(l)
    return np.stack([O.fft_process_long_range(cur[k], prev[k], lay, precision)[0] for k in range(cur.shape[0])])


def inside_np(l, pred, applied, kinds_per_pair):
    """[pairs, patches] bool: the clamp is inactive and the displaced previous window lies wholly in the patch's own cell; False in a
    constant cell"""
    out = np.zeros(pred.shape[:2], bool)
    cs = cells(l)
    for k in range(pred.shape[0]):
        for p in range(pred.shape[1]):
            c = cell_of(l, p)
            if kinds_per_pair[k][c][0] == "constant" or not np.array_equal(pred[k, p], applied[k, p]):
                continue
            x0, y0 = PC.origin_of(l, p)
            x, y = x0 - int(applied[k, p, 0]), y0 - int(applied[k, p, 1])
            cx0, cy0, cx1, cy1 = cs[c]
            out[k, p] = cx0 <= x and x + l.n <= cx1 and cy0 <= y and y + l.n <= cy1
    return out


def window_oracles(l, cur, disp, mask):
    """per pair and patch under `mask`: -O.phase_correlate(cur window, displaced prev window) at 64 and 32 bit (NaN elsewhere) and
    whether the f64 surface has a clear peak (second value outside the 5 x 5 window < half the peak)"""
    w64 = np.full(mask.shape + (2,), np.nan)
    w32 = np.full_like(w64, np.nan)
    clear = np.zeros(mask.shape, bool)
    for k, p in np.argwhere(mask):
        a, b = PC.window(l, cur[k], p), PC.window(l, disp[k], p)
        (x, y), d = O.phase_correlate(a, b, 64)
        w64[k, p] = (-x, -y)
        clear[k, p] = d["second_value"] < 0.5 * d["peak_value"]
        (x, y), _ = O.phase_correlate(a, b, 32)
        w32[k, p] = (-x, -y)
    return w64, w32, clear


Scene = namedtuple("Scene", "layout cur prev kinds coarse64 coarse32 pred applied disp inside w64 w32 clear")


@functools.lru_cache(maxsize=None)
def scene(name):
    l = BY_NAME[name]
    frames = [_paint(l, k) for k in range(N_PAIRS)]
    cur, prev = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    ks = [kinds(l, k) for k in range(N_PAIRS)]
    coarse64, coarse32 = _coarse(l, cur, prev, 64), _coarse(l, cur, prev, 32)
    pred = PC.c2f_pred_np(l, coarse64)
    applied = PC.applied_np(l, pred)
    disp = PC.displaced_np(l, prev, applied)
    inside = inside_np(l, pred, applied, ks)
    w64, w32, clear = window_oracles(l, cur, disp, inside)
    for a in (cur, prev, coarse64, coarse32, pred, applied, disp, inside, w64, w32, clear):
        a.setflags(write=False)
    return Scene(l, cur, prev, ks, coarse64, coarse32, pred, applied, disp, inside, w64, w32, clear)


def counted(s, k):
    """the patches of pair k whose cell is planted with a shift (the constant and the identical cell are not counted)"""
    return np.array([s.kinds[k][cell_of(s.layout, p)][0] == "shift" for p in range(PC.patches(s.layout))])


def lr_windows(l, cur, prev, p):
    """(cur, prev) quarter-image pixels of long-range patch p"""
    gxl = lr_grid(l)[0]
    qc, qp = O.resize_quarter(cur), O.resize_quarter(prev)
    x0, y0 = (p % gxl) * l.n, (p // gxl) * l.n
    return qc[y0:y0 + l.n, x0:x0 + l.n], qp[y0:y0 + l.n, x0:x0 + l.n]


Gate = namedtuple("Gate", "layout cur prev kinds coarse64 responses threshold")


@functools.lru_cache(maxsize=None)
def gate_case(name):
    """one extra pair whose cell GATE_CELL shows an unrelated texture in the previous frame; the f64 oracle's long-range responses and a
    threshold half way between that cell's and the smallest of the others"""
    l = BY_NAME[name]
    cur, prev = (f[None] for f in _paint(l, 3, unrelated=GATE_CELL))
    coarse64 = _coarse(l, cur, prev, 64)
    responses = np.array([O.phase_correlate(*lr_windows(l, cur[0], prev[0], p), 64)[1]["response"] for p in range(len(cells(l)))])
    others = np.delete(responses, GATE_CELL)
    threshold = float(0.5 * (responses[GATE_CELL] + others.min()))
    for a in (cur, prev, coarse64, responses):
        a.setflags(write=False)
    return Gate(l, cur, prev, kinds(l, 3), coarse64, responses, threshold)


# ---- coarse to fine on every pair route ----
ROUTE_SIZES = [64, 120, 128, 96, 160, 62, 200, 57, 24]
ROUTE_PLANTED = (24, -20)
ROUTE_PAIRS = 2
ROUTE_SEED = 43  # texture index of pair k: ROUTE_SEED + k, on the (1 6 1) blur (no spectral zero: tests/route_cases.py); the first from 40 on that
                 # keeps every long-range component 0.005 px off a rounding tie at every size (test_fft_pred_field_host.py)


def route_row(n):
    return R.default_table()[(R.PEAK_OPENCV, n)]


def route_fused(n):
    """the recorded table's word on whether a fused form exists: the family is TUNED at 32, 64 or 128, or pairs run on the half tile"""
    row = route_row(n)
    return (row[0] == "TUNED" and n in (32, 64, 128)) or row[2] > 0


def route_layout(n):
    return Layout(f"r_{n}", n, 4 * n, 4 * n, (4, 4), (0, 0), (n, n), 4 * n, R.variant(route_row(n)))


def route_clamped(n):
    """how many of the 16 patches the clamp holds back under the planted shift itself: column 0 (x0 - 24 < 0) and row 3 (y0 + 20 > 3 n)"""
    l = route_layout(n)
    return sum(PC.clamp_np(l, p, *ROUTE_PLANTED) != ROUTE_PLANTED for p in range(16))


Route = namedtuple("Route", "layout cur prev coarse64 coarse32 pred applied disp free w64 w32 clear")


@functools.lru_cache(maxsize=None)
def route_case(n):
    l = route_layout(n)
    frames = [synth.pair_np(ROUTE_SEED + k, l.h, l.w, *ROUTE_PLANTED, blur="mild") for k in range(ROUTE_PAIRS)]
    cur, prev = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    coarse64, coarse32 = _coarse(l, cur, prev, 64), _coarse(l, cur, prev, 32)
    pred = PC.c2f_pred_np(l, coarse64)
    applied = PC.applied_np(l, pred)
    disp = PC.displaced_np(l, prev, applied)
    free = (applied == pred).all(axis=-1)
    w64, w32, clear = window_oracles(l, cur, disp, np.ones(free.shape, bool))
    for a in (cur, prev, coarse64, coarse32, pred, applied, disp, free, w64, w32, clear):
        a.setflags(write=False)
    return Route(l, cur, prev, coarse64, coarse32, pred, applied, disp, free, w64, w32, clear)
