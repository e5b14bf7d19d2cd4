"""Inputs and CPU-oracle references of the block matchers' quality and match-gate tests (test_bm_quality_host.py, test_gpu_bm_quality.py).

A SHAPE is the smallest FastSpacedBMMethod geometry that reaches one branch of the two scan kernels (csrc/bm_kernel.hip); a CONTENT is a
batch of frame pairs on that shape. The reference of everything is the oracle's sad_all[block][ys][xs] (oracle_lib.bm_process(...,
want_sad=True)): min_sad = min, zero_sad = [r][r], max_sad = max; a block is valid iff min_sad <= max_min_sad and max_sad - min_sad >=
min_sad_range; the gated mode is oracle_lib.bm_histogram_top on the valid blocks. All integers, every comparison exact. Nothing here comes
from a GPU. Built once per process, shared, read-only."""
import functools

import numpy as np

import gate_cases as GC
import hard_content as HC
import oracle_lib as O
import quality_cases as Q

INVALID = -128  # MOF_BM_INVALID


class Shape:
    def __init__(self, name, block, radius, step, grid, scan16):
        self.name, self.block, self.radius, self.step, self.grid, self.scan16 = name, block, radius, step, grid, scan16
        S = block + step
        # FastSpacedBMMethod's geometry: grid = ((W - 2r) / S, (H - 2r) / S) (FastSpacedBMMethod_OCL.cpp:90)
        self.w, self.h = grid[0] * S + 2 * radius, grid[1] * S + 2 * radius
        self.blocks = grid[0] * grid[1]

    def oracle_cfg(self):
        c = O.bm_config_fast_spaced(self.w, self.h, self.block, self.step, self.radius)
        assert (c.grid_x, c.grid_y) == self.grid, (self.name, c.grid_x, c.grid_y)
        return c

    def engine(self, **kw):
        from mrs_optic_flow_amd import FastSpacedBMMethod

        e = FastSpacedBMMethod(self.block, self.radius, self.step, (self.h, self.w), **kw)
        assert (e.cfg.grid_x, e.cfg.grid_y) == self.grid
        return e

    def window(self, p):
        """(y0, x0, side) of block p's window in the previous frame"""
        by, bx = divmod(p, self.grid[0])
        S = self.block + self.step
        return by * S, bx * S, self.block + 2 * self.radius


SHAPES = {s.name: s for s in (
    # scan16 (block 16, even radius, step % 4 == 0)
    Shape("s16-r2", 16, 2, 0, (3, 2), True),     # one lane per block, the centre lane is xg = 0
    Shape("s16-r6", 16, 6, 4, (5, 2), True),     # R % 4 = 2: the centre SAD sits in the other 16-bit field pair
    Shape("s16-r8", 16, 8, 8, (17, 2), True),    # two waves of 9 and 8 blocks, idle lanes shadow the last block
    Shape("s16-r16", 16, 16, 8, (9, 2), True),   # c3's class: two waves of 5 and 4
    # the generic scan
    Shape("g8-r3", 8, 3, 0, (5, 4), False),      # D = 7: one padded x-shift; the last workgroup of a block row is ragged
    Shape("g32-r8", 32, 8, 0, (3, 3), False),    # c1's class
    Shape("g120-r21", 120, 21, 0, (1, 1), False),  # the reference default's block on a 162 x 162 frame: row flushes, sums above 2^16
    Shape("g12-r5", 12, 5, 0, (3, 2), False),    # odd CPD, block rows not 8-byte aligned
    # under MOF_BM_XB=2 the plan holds 7 blocks in 163 828 bytes of LDS: the quality form's 4 more bytes per block do not fit, it takes 6
    Shape("g100-r4", 100, 4, 0, (7, 1), False),
)}
# the same kernels on the routes only a knob selects: (shape, environment)
KNOBS = (("s16-r8", {"MOF_BM_GENERIC": "1"}), ("g32-r8", {"MOF_BM_XB": "1"}), ("g32-r8", {"MOF_BM_XB": "2"}), ("g32-r8", {"MOF_BM_XB": "3"}),
         ("g100-r4", {"MOF_BM_XB": "2"}))
CONTENTS = ("scenes", "hard", "directed")
CORNERS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (x, y) of the directed pairs' arg-max, in units of 2r


def _matched(s, seed):
    """cur = the blurred texture shifted by (3, -2) (clipped to the scan range) against prev, sigma = 2 noise on both"""
    rng = np.random.default_rng(seed)
    dx, dy = min(3, s.radius), -min(2, s.radius)
    base = Q._blurred(seed + 1000, s.h + 16, s.w + 16)
    prev = Q._noisy_u8(base[8:8 + s.h, 8:8 + s.w], rng)
    cur = Q._noisy_u8(base[8 + dy:8 + dy + s.h, 8 + dx:8 + dx + s.w], rng)
    return cur, prev


def _scenes(s):
    """pair 0 matched; pair 1 two unrelated views; pair 2 mixed: matched, with the window of block 0 of prev replaced by an unrelated view
    and the window of the last block by a constant (a single-block shape: the whole previous frame constant)"""
    c0, p0 = _matched(s, 11)
    c1, _ = _matched(s, 12)
    p1 = GC.unrelated(s.h, s.w, 13)
    c2, p2 = _matched(s, 14)
    p2 = p2.copy()
    y, x, n = s.window(s.blocks - 1)
    p2[y:y + n, x:x + n] = 90
    if s.blocks > 1:
        y, x, n = s.window(0)
        p2[y:y + n, x:x + n] = GC.unrelated(n, n, 15)
    return np.stack([c0, c1, c2]), np.stack([p0, p1, p2])


def _hard(s):
    """full-range noise against full-range noise; impulses against their own shift; a saturating pair (binary noise against its inverse,
    rolled: whole runs of |255 - 0|)"""
    hw = (s.h, s.w)
    c0, p0 = HC.uniform_noise(21, hw), HC.uniform_noise(22, hw)
    p1 = HC.impulses(23, (max(s.h, 52), max(s.w, 52)), pitch=9)[:s.h, :s.w]  # (its lattice needs 40 pixels; the small frames crop it)
    c1 = np.roll(p1, (min(1, s.radius), -min(2, s.radius)), axis=(0, 1))
    c2 = HC.binary_noise(24, hw)
    p2 = np.roll(255 - c2, (1, 1), axis=(0, 1))
    return np.stack([c0, c1, c2]).astype(np.uint8), np.stack([p0, p1, p2]).astype(np.uint8)


def _directed(s):
    """four pairs: a dark cur against a prev that brightens toward one corner of every window, which puts the arg-MAX of every block at
    (0, 0), (2r, 0), (0, 2r), (2r, 2r) in turn -- the xs = 2R column of scan16 and the padded x-shift group of the generic scan are each
    the unique maximum at least once (test_bm_quality_host.py asserts that from the oracle)"""
    rx = np.arange(s.w) * 255 // (s.w - 1)
    ry = np.arange(s.h) * 255 // (s.h - 1)
    prev = []
    for cx, cy in CORNERS:
        x = rx if cx else rx[::-1]
        y = ry if cy else ry[::-1]
        prev.append(((x[None, :] + y[:, None]) // 2).astype(np.uint8))
    return np.zeros((4, s.h, s.w), np.uint8), np.stack(prev)


class Batch:
    """.cur, .prev [pairs, H, W]; the oracle's .dx, .dy [pairs, gy, gx], .mode [pairs, 8], .sad [pairs, blocks, D, D] and
    .quality [pairs, gy, gx, 3] uint32"""

    def __init__(self, shape, content, cur, prev):
        self.shape, self.content, self.cur, self.prev = shape, content, np.ascontiguousarray(cur), np.ascontiguousarray(prev)
        cfg, r = shape.oracle_cfg(), shape.radius
        dx, dy, sad = [], [], []
        for c, p in zip(self.cur, self.prev):
            x, y, _, sa = O.bm_process(c, p, cfg, want_sad=True)
            dx.append(x), dy.append(y), sad.append(sa)
        self.dx, self.dy, self.sad = np.stack(dx), np.stack(dy), np.stack(sad)
        flat = self.sad.reshape(len(self.cur), shape.blocks, -1)
        q = np.stack([flat.min(-1), self.sad[:, :, r, r], flat.max(-1)], axis=-1)
        self.quality = q.astype(np.uint32).reshape(len(self.cur), shape.grid[1], shape.grid[0], 3)
        self.mode = self.gated(0xFFFFFFFF, 0)[2]
        for a in (self.cur, self.prev, self.dx, self.dy, self.sad, self.quality, self.mode):
            a.setflags(write=False)

    def valid(self, max_min_sad, min_sad_range):
        q = self.quality.astype(np.int64)
        return (q[..., 0] <= max_min_sad) & (q[..., 2] - q[..., 0] >= min_sad_range)

    def gated(self, max_min_sad, min_sad_range):
        """(dx, dy, mode [pairs, 8], n_invalid [pairs]) under the gate, from the oracle alone"""
        v = self.valid(max_min_sad, min_sad_range)
        dx, dy = np.where(v, self.dx, INVALID).astype(np.int8), np.where(v, self.dy, INVALID).astype(np.int8)
        mode = np.zeros((len(dx), 8), np.int8)
        for k in range(len(dx)):
            if v[k].any():
                mode[k, 0:6:2] = O.bm_histogram_top(self.dx[k][v[k]], self.shape.radius)
                mode[k, 1:6:2] = O.bm_histogram_top(self.dy[k][v[k]], self.shape.radius)
            else:
                mode[k, :6] = INVALID
        return dx, dy, mode, (~v).reshape(len(dx), -1).sum(-1).astype(np.int32)

    def thresholds(self):
        """The gate of the scenes batch, from the oracle's own values: max_min_sad halfway between the largest min_sad of the matched pair
        (pair 0) and the smallest of the unrelated pair (pair 1), min_sad_range halfway between the largest range of the unrelated pair and
        the smallest of the matched one. Returns (max_min_sad, min_sad_range, the four figures)."""
        assert self.content == "scenes"
        q = self.quality.astype(np.int64).reshape(len(self.cur), -1, 3)
        m_lo, m_hi = int(q[0, :, 0].max()), int(q[1, :, 0].min())
        rng = q[..., 2] - q[..., 0]
        r_lo, r_hi = int(rng[1].max()), int(rng[0].min())
        return (m_lo + m_hi) // 2, (r_lo + r_hi + 1) // 2, (m_lo, m_hi, r_lo, r_hi)


_BUILD = {"scenes": _scenes, "hard": _hard, "directed": _directed}


@functools.lru_cache(maxsize=None)
def batch(shape_name, content):
    s = SHAPES[shape_name]
    return Batch(s, content, *_BUILD[content](s))


@functools.lru_cache(maxsize=None)
def constant_block_method():
    """BlockMethod(52, 16, 2) on a constant pair: every block's first minimum is shift index 0, so every block reports (-r, -r)"""
    cur = np.full((1, 52, 52), 77, np.uint8)
    return cur, cur.copy()


@functools.lru_cache(maxsize=None)
def bgr_scenes(shape_name):
    """the scenes batch as BGR8 frames (three noisy copies of each gray frame) and the Batch of their CV_RGB2GRAY conversion"""
    s, b = SHAPES[shape_name], batch(shape_name, "scenes")
    rng = np.random.default_rng(31)

    def colour(f):
        return np.clip(f[..., None].astype(np.int16) + rng.integers(-9, 10, f.shape + (3,)), 0, 255).astype(np.uint8)

    cur, prev = colour(b.cur), colour(b.prev)
    gray = lambda a: np.stack([O.rgb2gray(f) for f in a])  # noqa: E731
    return cur, prev, Batch(s, "scenes", gray(cur), gray(prev))
