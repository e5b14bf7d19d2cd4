"""The reference's OpenCL text executed on the CPU (oracle/cl_host.h, oracle/_ref/libref_*.so): ctypes access, and the ONE list of
cases that tests/test_ref_cl_host.py runs and tests/golden/make_ref_cl_fixtures.py records a subset of.

Everything here is deterministic (seeded numpy integer draws, integer image arithmetic), so the recorded fixtures can be regenerated
and compared byte for byte. Helper module: it holds no tests."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_OUT = os.path.join(O.ORACLE_DIR, "_ref")
PEAK_SIZES = (32, 64, 120)
FIELD = 7  # the far patch origin of every peak case: the last patch of a FIELD x FIELD field

_bm = None
_peak = {}


def reference_checkout_present() -> bool:
    d = subprocess.check_output(["make", "-C", O.ORACLE_DIR, "-s", "print-ref-dir"], text=True).strip()
    return os.path.exists(os.path.join(d, "src", "FastSpacedBMMethod.cl")) and os.path.exists(os.path.join(d, "cl", "FftMethod.cl"))


def library_paths():
    return [os.path.join(REF_OUT, "libref_bm_cl.so")] + [os.path.join(REF_OUT, f"libref_fft_peak_{n}.so") for n in PEAK_SIZES]


def usable() -> bool:
    return all(os.path.exists(p) for p in library_paths())


def bm_lib():
    global _bm
    if _bm is None:
        L = C.CDLL(os.path.join(REF_OUT, "libref_bm_cl.so"))
        L.ref_bm_cl.restype = C.c_int
        L.ref_bm_cl.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4
        _bm = L
    return _bm


def peak_lib(n: int):
    if n not in _peak:
        L = C.CDLL(os.path.join(REF_OUT, f"libref_fft_peak_{n}.so"))
        L.ref_fft_peak.restype = C.c_int
        L.ref_fft_peak.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.ref_fft_peak_params.restype = None
        L.ref_fft_peak_params.argtypes = [C.c_void_p]
        _peak[n] = L
    return _peak[n]


# ---- block matching ----------------------------------------------------------------------------------------------------

class BmCase:
    def __init__(self, name, cur, prev, block, step, radius, scan_block=None):
        self.name, self.block, self.step, self.radius = name, int(block), int(step), int(radius)
        self.cur = np.ascontiguousarray(cur, np.uint8)
        self.prev = np.ascontiguousarray(prev, np.uint8)
        assert self.cur.shape == self.prev.shape
        self.scan_block = int(scan_block) if scan_block else 2 * self.radius + 1
        h, w = self.cur.shape
        s = self.block + self.step
        self.grid = ((w - 2 * self.radius) // s, (h - 2 * self.radius) // s)  # (x, y)
        # what the CPU host is asked to run at once: one OptFlow work-group, and the Histogram's single group
        assert self.scan_block ** 2 <= 1100 and self.grid[0] * self.grid[1] <= 1100, name
        assert 2 * self.radius + 1 < 50 and self.grid[0] >= 1 and self.grid[1] >= 1, name


def frame_size(block, step, radius, gx, gy, extra=(0, 0)):
    """(h, w) of the smallest frame with a gx x gy grid, plus `extra` (x, y) pixels that no block reaches (< block + step)."""
    s = block + step
    return (2 * radius + gy * s + extra[1], 2 * radius + gx * s + extra[0])


def bm_reference(c: BmCase):
    """The reference text's (dx[gy, gx], dy[gy, gx], top3x, top3y)."""
    gx, gy = c.grid
    dx, dy = np.full(gx * gy, 99, np.int8), np.full(gx * gy, 99, np.int8)
    o9x, o9y = np.full(9, 99, np.int8), np.full(9, 99, np.int8)
    h, w = c.cur.shape
    rc = bm_lib().ref_bm_cl(c.cur.ctypes.data, c.prev.ctypes.data, w, h, c.block, c.step, c.radius, c.scan_block,
                            dx.ctypes.data, dy.ctypes.data, o9x.ctypes.data, o9y.ctypes.data)
    if rc:
        raise ValueError(f"ref_bm_cl rc={rc} ({c.name})")
    # the nine candidates are the cross product of the two top-3 lists (x-major): check that, then keep the lists
    assert (o9x.reshape(3, 3) == o9x[0:9:3, None]).all() and (o9y.reshape(3, 3) == o9y[None, 0:3]).all()
    return dx.reshape(gy, gx), dy.reshape(gy, gx), o9x[0:9:3].copy(), o9y[0:3].copy()


def bm_oracle(c: BmCase):
    h, w = c.cur.shape
    cfg = O.bm_config_fast_spaced(w, h, c.block, c.step, c.radius)
    assert (cfg.grid_x, cfg.grid_y) == c.grid
    dx, dy, _ = O.bm_process(c.cur, c.prev, cfg)
    return dx, dy, O.bm_histogram_top(dx, c.radius, 3), O.bm_histogram_top(dy, c.radius, 3)


def _shifted_pair(rng, h, w, sx, sy, lo=0, hi=256):
    """prev = a random field, cur = the same field displaced so that the block scan's best candidate is (sx, sy)."""
    pad = 32
    big = rng.integers(lo, hi, (h + 2 * pad, w + 2 * pad), dtype=np.uint8)
    prev = big[pad:pad + h, pad:pad + w]
    cur = big[pad + sy:pad + sy + h, pad + sx:pad + sx + w]  # cur(y, x) = prev(y + sy, x + sx)
    return cur.copy(), prev.copy()


def frames_from_shifts(rng, shifts_x, shifts_y, block, radius):
    """A frame pair whose block (bx, by) matches exactly at (shifts_x[by][bx], shifts_y[by][bx]): windows do not overlap
    (step = 2 radius), each window is its own random texture, the current block is cut out of it at the wanted candidate."""
    sx, sy = np.asarray(shifts_x), np.asarray(shifts_y)
    gy, gx = sx.shape
    step = 2 * radius
    s = block + step
    h, w = frame_size(block, step, radius, gx, gy)
    prev = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cur = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for by in range(gy):
        for bx in range(gx):
            x0, y0 = bx * s, by * s
            xs, ys = int(sx[by, bx]) + radius, int(sy[by, bx]) + radius
            cur[y0 + radius:y0 + radius + block, x0 + radius:x0 + radius + block] = prev[y0 + ys:y0 + ys + block, x0 + xs:x0 + xs + block]
    return cur, prev, step


def bm_sweep_cases(count=160, seed=20261021):
    """Seeded small geometries: blocks 4 .. 16, step 0 / 3 / 4, radius 2 .. 21, grids of 2 .. 24 blocks, four kinds of content,
    scan_block equal to the diameter (one pass of the kernel's loops) or smaller (its `repetitions` loops)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        block = int(rng.integers(4, 17))
        step = int(rng.choice([0, 3, 4]))
        radius = int(rng.integers(2, 22))
        gx, gy = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        if gx * gy < 2:
            gx = 2
        h, w = frame_size(block, step, radius, gx, gy, (int(rng.integers(0, block + step)), int(rng.integers(0, block + step))))
        kind = ("shifted", "alphabet", "constant+6", "noise")[k % 4]
        if kind == "shifted":
            cur, prev = _shifted_pair(rng, h, w, int(rng.integers(-radius, radius + 1)), int(rng.integers(-radius, radius + 1)))
        elif kind == "alphabet":  # three values: exact SAD ties everywhere
            cur, prev = rng.integers(0, 3, (h, w), dtype=np.uint8) * 40, rng.integers(0, 3, (h, w), dtype=np.uint8) * 40
        elif kind == "constant+6":  # a constant pair, one pixel of the previous frame 6 higher
            cur, prev = np.full((h, w), 77, np.uint8), np.full((h, w), 77, np.uint8)
            prev[int(rng.integers(0, h)), int(rng.integers(0, w))] += 6
        else:
            cur, prev = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
        d = 2 * radius + 1
        full_ok = d * d <= 1100
        sb = d if (full_ok and k % 3 == 0) else int(rng.integers(1, min(d, 33)))
        out.append(BmCase(f"sweep{k:03d}-{kind}-b{block}s{step}r{radius}g{gx}x{gy}sb{sb}", cur, prev, block, step, radius, sb))
    return out


def bm_low_contrast_case(radius=5, block=8):
    """Two blocks side by side with disjoint windows; in each, one pixel of the previous frame is raised so that the centre SAD
    is exactly `gap` above the minimum: gap 5 = 0.2 r^2 (zeroed: the kernel compares `<=` with a double), gap 6 (kept)."""
    step = 2 * radius
    s = block + step
    h, w = frame_size(block, step, radius, 2, 1)
    cur, prev = np.full((h, w), 100, np.uint8), np.full((h, w), 100, np.uint8)
    prev[radius, radius] += 5      # seen by block 0's candidates with xs <= r and ys <= r, the centre among them
    prev[radius, s + radius] += 6  # the same pixel of block 1's window
    return BmCase(f"low-contrast-r{radius}", cur, prev, block, step, radius)


def bm_engineered_cases():
    out = []
    rng = np.random.default_rng(77)
    # constant pairs: every SAD ties (first minimum (-r, -r)), and the low-contrast rule then writes (0, 0)
    for block, step, radius, value in ((4, 0, 2, 0), (8, 4, 5, 90), (16, 8, 8, 255), (12, 3, 16, 17)):
        h, w = frame_size(block, step, radius, 3, 2, (1, 2))
        f = np.full((h, w), value, np.uint8)
        out.append(BmCase(f"constant-b{block}r{radius}", f, f, block, step, radius))
    out.append(bm_low_contrast_case())
    # periodic texture: several candidates with SAD 0 and a large centre SAD -- the first in row-major order must win
    for block, step, radius, period, sb in ((8, 0, 6, (3, 4), 13), (16, 8, 9, (5, 3), 16), (4, 3, 12, (7, 2), 3)):
        h, w = frame_size(block, step, radius, 3, 2)
        tile = rng.integers(0, 256, (period[1], period[0]), dtype=np.uint8)
        big = np.tile(tile, (h // period[1] + 3, w // period[0] + 3))
        out.append(BmCase(f"periodic-b{block}r{radius}", big[1:1 + h, 2:2 + w], big[:h, :w], block, step, radius, sb))
    # histograms: engineered count ties between bins, fewer than three occupied bins, modes at the ends of the range
    r = 4
    designs = {
        "hist-ties-3-bins": ([[2, 2, -1], [-1, 3, 3]], [[0, -4, 0], [-4, 4, 4]]),
        "hist-ties-and-singles": ([[2, 2, -1, -1], [0, 3, 3, -3]], [[1, 1, 1, -2], [-2, -2, 4, 0]]),
        "hist-one-bin": ([[1, 1], [1, 1]], [[-4, -4], [-4, -4]]),
        "hist-two-bins": ([[4, 4, -4]], [[-3, 2, 2]]),
        "hist-two-bins-tied": ([[3, -2]], [[-4, 4]]),
        "hist-all-distinct": ([[-4, -3, -2, -1, 0, 1, 2, 3, 4]], [[4, 3, 2, 1, 0, -1, -2, -3, -4]]),
    }
    for name, (sx, sy) in designs.items():
        cur, prev, step = frames_from_shifts(rng, sx, sy, 8, r)
        out.append(BmCase(name, cur, prev, 8, step, r))
    # scan_block in {2r + 1, 16 for r > 7, 3}; radius 21 and 24 (diameter 43 / 49, just inside the text's arrays of 50)
    for radius, sbs in ((3, (7, 3)), (8, (17, 16, 3)), (16, (33, 16, 3)), (21, (16, 3)), (24, (16, 3))):
        for sb in sbs:
            block = 8 if radius > 16 else 12
            h, w = frame_size(block, 4, radius, 2, 2, (3, 1))
            cur, prev = _shifted_pair(rng, h, w, -radius if sb == 3 else radius - 1, radius if sb == 16 else 1 - radius)
            out.append(BmCase(f"scanblock-r{radius}-sb{sb}", cur, prev, block, 4, radius, sb))
    # saturating content: 0 against 255 (every SAD 255 b^2), and a 0 / 255 texture displaced (differences of exactly 255)
    for block in (16, 32):
        radius = 4
        h, w = frame_size(block, 0, radius, 2, 2)
        out.append(BmCase(f"saturated-const-b{block}", np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8), block, 0, radius))
        cur, prev = _shifted_pair(rng, h, w, 3, -2, 0, 2)
        out.append(BmCase(f"saturated-texture-b{block}", cur * 255, prev * 255, block, 0, radius))
        cur = rng.integers(0, 2, (h, w), dtype=np.uint8) * 255
        out.append(BmCase(f"saturated-inverse-b{block}", cur, 255 - cur, block, 0, radius, 5))
    return out


def bm_gpu_cases():
    """The geometries tests/test_gpu_ref_cl.py runs on the device (all recorded): the register-resident 16 x 16 scan at three
    radii, and the generic scan's three forms. Grids >= 2 blocks, frames <= 200 x 330."""
    rng = np.random.default_rng(5150)
    out = []
    for radius in (2, 8, 16):
        h, w = frame_size(16, 8, radius, 5, 3, (5, 2))
        cur, prev = _shifted_pair(rng, h, w, radius - 1, -radius)
        cur[:h // 2] = rng.integers(0, 3, (h // 2, w), dtype=np.uint8) * 9  # upper rows: ties and low contrast
        out.append(BmCase(f"gpu-scan16-r{radius}", cur, prev, 16, 8, radius))
    for name, block, step, radius, gx, gy in (("gpu-generic-8-blocks-per-group", 8, 4, 5, 9, 2), ("gpu-generic-ragged-row", 36, 4, 7, 3, 2),
                                              ("gpu-generic-flushed-sums", 64, 0, 3, 2, 2)):
        h, w = frame_size(block, step, radius, gx, gy, (1, 3))
        cur, prev = _shifted_pair(rng, h, w, -2, 3)
        prev[:, w // 2:] = rng.integers(0, 2, (h, w - w // 2), dtype=np.uint8) * 255  # right half: saturated noise
        out.append(BmCase(name, cur, prev, block, step, radius, 3 if block == 64 else None))
    return out


def bm_one_block_cases():
    """1 x 1 grids: the reference text sorts its Y histogram in work-item 1, which such a launch does not have."""
    rng = np.random.default_rng(11)
    out = []
    for radius, sx, sy in ((4, 2, 3), (6, -5, -1), (3, 0, 3)):
        cur, prev, step = frames_from_shifts(rng, [[sx]], [[sy]], 8, radius)
        c = BmCase(f"one-block-r{radius}", cur, prev, 8, step, radius)
        c.true_shift = (sx, sy)
        out.append(c)
    return out


def bm_recorded_cases():
    """What tests/golden/ref_cl_bm.npz holds."""
    eng = [c for c in bm_engineered_cases() if c.name.startswith(("low-contrast", "hist-", "periodic-b8", "saturated-texture-b16",
                                                                  "scanblock-r21-sb16", "scanblock-r24-sb3", "constant-b8"))]
    sweep = [c for c in bm_sweep_cases() if c.block % 4 == 0][:12]  # (the kernels take blocks that are multiples of 4)
    return bm_gpu_cases() + eng + sweep + bm_one_block_cases()[:1]


# ---- the peak stage -----------------------------------------------------------------------------------------------------

def peak_params(n: int):
    """(kercn, WGS, WGS2_ALIGNED) as the reference's host derives them for patch size n (FftMethod.cpp:481-539, :790, :333-339),
    restated: the 2-power part of n goes in radix-8 / 4 / 2 steps (the 4 and 2 steps blocked by 12 / 8, resp. 10 / 8 / 6 / 4),
    every odd prime factor in one step (3 blocked by 12 / 9 / 6, 5 by 10); kercn is the smallest radix x block."""
    p2 = n & -n
    odd, f, factors = n // p2, 3, []
    while odd > 1:
        while odd % f == 0:
            factors.append(f)
            odd //= f
        f += 2
    mins = []
    m = 1
    while p2 > 1 and m < p2:
        if 8 * m <= p2:
            radix, block = 8, 1
        elif 4 * m <= p2:
            radix, block = 4, 3 if n % 12 == 0 else 2 if n % 8 == 0 else 1
        else:
            radix, block = 2, 5 if n % 10 == 0 else 4 if n % 8 == 0 else 3 if n % 6 == 0 else 2 if n % 4 == 0 else 1
        mins.append(radix * block)
        m *= radix
    for f in factors:
        block = 1
        if f == 3:
            block = 4 if n % 12 == 0 else 3 if n % 9 == 0 else 2 if n % 6 == 0 else 1
        elif f == 5:
            block = 2 if n % 10 == 0 else 1
        mins.append(f * block)
    kercn = min(mins)
    wgs = n // kercn
    w2 = 1
    while w2 < wgs:
        w2 <<= 1
    return kercn, wgs, w2 >> 1


def peak_reference(surface: np.ndarray, xvec: int, yvec: int, frame=None) -> np.ndarray:
    """The reference text's two result floats for `surface` placed as patch (xvec, yvec) of a FIELD x FIELD frame whose other
    patches hold large values (a read outside the patch would win the arg-max)."""
    n = surface.shape[0]
    if frame is None:
        frame = np.full((FIELD * n, FIELD * n), 1000.0, np.float32)
    frame[yvec * n:(yvec + 1) * n, xvec * n:(xvec + 1) * n] = surface
    out = np.full(2, np.nan, np.float32)
    rc = peak_lib(n).ref_fft_peak(frame.ctypes.data, frame.strides[0], frame.shape[1], n, xvec, yvec, out.ctypes.data)
    frame[yvec * n:(yvec + 1) * n, xvec * n:(xvec + 1) * n] = 1000.0
    if rc:
        raise ValueError(f"ref_fft_peak rc={rc}")
    return out


def peak_oracle(surface: np.ndarray, xvec: int, yvec: int) -> np.ndarray:
    n = surface.shape[0]
    got = O.ocl_peak(surface, (xvec * n, yvec * n), 32)
    f = got.astype(np.float32)
    assert (f.astype(np.float64) == got).all()  # the f32 oracle's results are floats
    return f


def patch_pairs(n: int, count=10, seed=4242):
    """uint8 patch pairs (cur, prev): a blocky random texture displaced by whole and half pixels, with noise; the last one is
    unrelated noise (no peak stands out: it fails the usual second-peak filter on purpose)."""
    rng = np.random.default_rng(seed + n)
    out = []
    for k in range(count):
        cells = rng.integers(0, 256, (n // 4 + 16, n // 4 + 16), dtype=np.uint8)
        big = np.kron(cells, np.ones((4, 4), np.uint8)).astype(np.int32)
        # (plus per-pixel detail: a purely blocky patch has spectral bins that are exactly zero, the Nyquist ones among them,
        # and the model's 1 / (a b) at the four real-only bins is then infinite)
        big = (3 * big + rng.integers(0, 256, big.shape)) // 4
        sx, sy = int(rng.integers(-6, 7)), int(rng.integers(-6, 7))
        hx, hy = int(rng.integers(0, 2)), int(rng.integers(0, 2))  # half-pixel part: the mean of two whole displacements
        o = 32
        prev = big[o:o + n, o:o + n]
        a = big[o - sy:o - sy + n, o - sx:o - sx + n]
        b = big[o - sy - hy:o - sy - hy + n, o - sx - hx:o - sx - hx + n]
        cur = (a + b + 1) // 2
        amp = (0, 2, 6, 12, 25)[k % 5]
        if amp:
            cur = cur + rng.integers(-amp, amp + 1, (n, n))
            prev = prev + rng.integers(-amp, amp + 1, (n, n))
        if k == count - 1:
            cur = rng.integers(0, 256, (n, n))
        out.append((np.clip(cur, 0, 255).astype(np.uint8), np.clip(prev, 0, 255).astype(np.uint8)))
    return out


def pair_surface(cur: np.ndarray, prev: np.ndarray):
    """The oracle's own f32 surface for a patch pair, and its diagnostic."""
    _, diag, surf = O.phase_correlate_ocl(cur.astype(np.float32), prev.astype(np.float32), (0, 0), 55, 32, want_surface=True)
    return surf, diag


def _background(rng, n):
    return (rng.integers(-100, 101, (n, n)) / np.float32(10000.0)).astype(np.float32)  # +-0.01, both signs


def _bump(s, y, x, rng, peak=1.0):
    n = s.shape[0]
    for yy in range(max(0, y - 2), min(n, y + 3)):
        for xx in range(max(0, x - 2), min(n, x + 3)):
            s[yy, xx] = np.float32(int(rng.integers(5, 60)) / 100.0)
    s[y, x] = np.float32(peak)


def synthetic_surfaces(n: int):
    """(name, surface) pairs: see the list in tests/test_ref_cl_host.py."""
    rng = np.random.default_rng(900 + n)
    kercn, wgs, w2 = peak_params(n)
    out = []
    mid = n // 2 - 3
    # peaks on every corner and edge, one to three pixels inside each (the refine window clamps to 4 .. 7 cells per axis; at 3 and
    # n - 4 it is whole for the first time, at n - 3 an off-by-one clamp would read the next row), and the interior
    edge = (0, 1, 2, 3, mid, n - 4, n - 3, n - 2, n - 1)
    for y in edge:
        for x in edge:
            s = _background(rng, n)
            _bump(s, y, x, rng)
            out.append((f"peak-y{y}-x{x}", s))
    # a maximum that only one work-item holds, for every work-item (lid >= WGS2_ALIGNED merges before the tree)
    for lid in range(wgs):
        s = _background(rng, n)
        _bump(s, int(rng.integers(3, n - 3)), lid * kercn + int(rng.integers(0, kercn)), rng)
        out.append((f"lid{lid}", s))
    # exact ties in one row: the lowest index wins, whichever work-items hold the members (same item, both tree halves, the
    # lid >= WGS2_ALIGNED merge against its partner slot and against another slot)
    lids = sorted({0, 1, w2 - 1, w2, min(w2 + 1, wgs - 1), wgs - 1})
    row = n // 2 + 2
    for i, la in enumerate(lids):
        for lb in lids[i:]:
            xa, xb = la * kercn + 1, lb * kercn + kercn - 2
            if xb - xa < 6:
                continue  # the two bumps must not overlap
            for first_is_real in (True, False):
                s = _background(rng, n)
                # the bump that must NOT be chosen gets the larger neighbourhood, so a wrong choice moves the centroid
                _bump(s, row, xa, rng)
                _bump(s, row, xb, rng)
                s[row, xa + 1 if first_is_real else xb - 1] = np.float32(0.9)
                out.append((f"row-tie-lid{la}-lid{lb}-{'a' if first_is_real else 'b'}", s))
    s = _background(rng, n)
    _bump(s, row, 2 * kercn + 1, rng)
    s[row, 2 * kercn + 4] = np.float32(1.0)  # two members in one work-item's stretch
    out.append(("row-tie-same-item", s))
    # exact ties across rows: the first row wins even where the later row's member has the lower column
    for (ya, xa), (yb, xb) in (((5, n - 6), (n - 8, 4)), ((n // 2, n // 2), (n // 2 + 1, 3)), ((0, n - 1), (n - 1, 0)), ((2, 9), (20, 9))):
        s = _background(rng, n)
        _bump(s, ya, xa, rng)
        _bump(s, yb, xb, rng)
        out.append((f"cross-row-tie-{ya}-{xa}-{yb}-{xb}", s))
    # a three-way tie spread over both kinds of work-item and two rows
    s = _background(rng, n)
    for y, x in ((row, (wgs - 1) * kercn + 2), (row, 3), (row - 9, w2 * kercn)):
        _bump(s, y, x, rng)
    out.append(("three-way-tie", s))
    # nothing positive in the window: the sum stays FLT_EPSILON and the centroid 0
    s = -np.abs(_background(rng, n)) - np.float32(0.5)
    s[n // 3, n // 4] = np.float32(-0.25)
    out.append(("all-negative", s))
    s = -np.abs(_background(rng, n)) - np.float32(0.5)
    s[7, n - 9] = np.float32(0.0)
    out.append(("max-is-zero", s))
    s = -np.abs(_background(rng, n)) - np.float32(0.5)
    s[n - 4, 6] = np.float32(1e-30)  # one tiny positive value: 1e-30 + FLT_EPSILON rounds to FLT_EPSILON
    out.append(("one-tiny-positive", s))
    out.append(("all-zero", np.zeros((n, n), np.float32)))
    out.append(("constant-positive", np.full((n, n), 0.125, np.float32)))  # everything ties: (0, 0) wins, window 4 x 4
    return out


def peak_cases(n: int):
    """Every surface of size n: (name, surface, from_pair)."""
    out = []
    for k, (cur, prev) in enumerate(patch_pairs(n)):
        out.append((f"pair{k}", pair_surface(cur, prev)[0], True))
    return out + [(name, s, False) for name, s in synthetic_surfaces(n)]


def recorded_synthetic(n: int):
    """The synthetic surfaces tests/golden/ref_cl_fft_peak.npz holds: every tie / sign / work-item case, and of the 81 peak
    positions those with both coordinates among (0, 3, mid, n - 3, n - 1)."""
    keep = {0, 3, n // 2 - 3, n - 3, n - 1}
    out = []
    for name, s in synthetic_surfaces(n):
        if name.startswith("peak-"):
            y, x = int(name.split("-")[1][1:]), int(name.split("-")[2][1:])
            if y not in keep or x not in keep:
                continue
        out.append((name, s))
    return out


PEAK_ORIGINS = ((0, 0), (FIELD - 1, FIELD - 1), (2, 5))
