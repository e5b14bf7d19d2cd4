"""The cases of tests/test_gpu_fft_k1_lone_lane.py, shared with tests/golden/make_k1_lone_lane.py (which records what the library in use
computes for them). They walk what decides how the wave that holds the maximum of a 64 x 64 surface comes by its (value, index) pair
behind the arg-max barrier of K1 (csrc/pc_kernel.hip, holder_pair): ONE lane of the wave at the maximum -- the pair is read out of that
lane --, one lane holding it several times -- the lane's equality mask decides by its fixed order --, two lanes of one wave, several
waves; and the two cross-power forms met in rows 0 and 32 of the spectrum, which wave 0 packs alone. Through every record form.

Who holds what (csrc/pc_passes.hpp, col_pass_inv): wave w owns the un-shifted columns [8 w, 8 w + 8) and those + 32; lane 8 x + c of it
holds the rows y = x + 8 k, k = 0 .. 7, of the columns 8 w + c (.x) and 8 w + c + 32 (.y). Its fixed order starts with k = 4 .. 7, the
un-shifted rows from 32 on, and ends with k = 0 .. 3, the rows below 32.

A case is (name, run): run(g, dev) -> {key: numpy array}, g the dict of input arrays of the fixture (make_inputs). One 64 x 64 patch per
frame; the generators and the runners are those of tests/k1_finish_cases.py."""
import os

import numpy as np

import k1_finish_cases as K

N = K.N
# a lone lane in each wave, both column halves, peak rows below 32 and from 32 on -- whichever sign the roll comes out with: the columns
# 3 + 8 j and 64 - (3 + 8 j) both cover w = 0 .. 3 twice, the rows 5 | 59 and 41 | 23 both halves of the lane's order
LONE_ROLLS = [(dy, 3 + 8 * j) for dy in (5, 41) for j in range(8)]
# exact periods (period_y, period_x) and the roll of cur against prev; 64 = none along that axis
IN_LANE = (((64, 32), (3, 1)), ((64, 32), (40, 9)), ((32, 64), (3, 1)), ((32, 64), (9, 40)), ((32, 32), (3, 1)), ((32, 32), (20, 29)))
TWO_LANES = (((4, 64), (1, 2)), ((4, 64), (2, 37)), ((4, 64), (0, 60)))
OFFSET_PRED = K.OFFSET_PRED


def _tiled(rng, periods, roll, shape=(N, N), channels=()):
    py, px = periods
    t = np.tile(rng.integers(0, 256, (py, px) + channels, dtype=np.uint8), (shape[0] // py, shape[1] // px) + (1,) * len(channels))
    return np.roll(t, roll, axis=(0, 1)), t


def _stack(pairs):
    return np.stack([c for c, _ in pairs]), np.stack([p for _, p in pairs])


def exact_periods(img):
    """(period_y, period_x) of an image [H, W(, C)]: the smallest divisors of its sides by which a roll leaves it unchanged"""
    return tuple(next(d for d in range(1, img.shape[ax] + 1) if img.shape[ax] % d == 0 and np.array_equal(np.roll(img, d, axis=ax), img))
                 for ax in (0, 1))


def make_inputs():
    rng = np.random.default_rng(20261023)
    g = {}
    g["lone_cur"], g["lone_prev"] = K._pairs(rng, LONE_ROLLS)
    g["inlane_cur"], g["inlane_prev"] = _stack([_tiled(rng, per, roll) for per, roll in IN_LANE])
    g["twolanes_cur"], g["twolanes_prev"] = _stack([_tiled(rng, per, roll) for per, roll in TWO_LANES])
    g["tie_cur"], g["tie_prev"] = K._ties(rng)  # constant / zero pairs, period 8 (several waves), period 32 and 16
    # rows 0 and 32 of the spectrum with both cross-power forms: the committed inputs of tests/test_gpu_fft_xpow_paths.py (the period-4
    # pattern and the 8 x 8 tile under one raised pixel: empty bins, row 0 among them, beside large ones), a constant image against
    # texture both ways, and a texture of period 2 along x -- every odd bin of every spectrum row exactly empty
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    xp = [np.load(os.path.join(gold, f"xpow_paths_{name}_n64.npz")) for name in ("mixed", "tile")]
    tex = rng.integers(0, 256, (N, N), dtype=np.uint8)
    extra = [(np.full((N, N), 143, np.uint8), tex), (tex, np.full((N, N), 7, np.uint8)), _tiled(rng, (64, 2), (5, 1))]
    g["xpow_cur"] = np.concatenate([x["cur"] for x in xp] + [np.stack([c for c, _ in extra])])
    g["xpow_prev"] = np.concatenate([x["prev"] for x in xp] + [np.stack([p for _, p in extra])])
    # every other record form: lone lanes and an in-lane tie each
    g["bgr_cur"], g["bgr_prev"] = (np.concatenate(t) for t in zip(
        K._pairs(rng, LONE_ROLLS[1::3], (N, N, 3)), _stack([_tiled(rng, (32, 32), (3, 1), channels=(3,)), _tiled(rng, (4, 64), (1, 2), channels=(3,))])))
    c, p = (np.concatenate(t) for t in zip(
        K._pairs(rng, [(2 * dy, 2 * dx) for dy, dx in LONE_ROLLS[2::5]], (128, 128)),
        _stack([_tiled(rng, (64, 64), (6, 2), (128, 128)), _tiled(rng, (8, 128), (2, 4), (128, 128))])))  # (half these periods at quarter resolution)
    g["lr_cur"], g["lr_prev"] = np.kron(c, np.ones((1, 2, 2), np.uint8)), np.kron(p, np.ones((1, 2, 2), np.uint8))
    g["off_cur"], g["off_prev"] = K._pairs(rng, LONE_ROLLS[:4], (80, 80))
    g["off_bgr_cur"], g["off_bgr_prev"] = K._pairs(rng, LONE_ROLLS[12:], (80, 80, 3))
    g["pred"] = OFFSET_PRED
    return g


def check_inputs(g):
    """what the tie cases claim about their inputs, exactly (numpy, no GPU)"""
    for (per, _), c, p in zip(IN_LANE, g["inlane_cur"], g["inlane_prev"]):
        assert exact_periods(c) == per and exact_periods(p) == per, (per, exact_periods(c), exact_periods(p))
    for (per, _), c, p in zip(TWO_LANES, g["twolanes_cur"], g["twolanes_prev"]):
        assert exact_periods(c) == per == exact_periods(p) == (4, 64), (per, exact_periods(c), exact_periods(p))
    for k, per in ((4, (8, 8)), (5, (8, 8)), (6, (32, 32)), (7, (32, 32)), (8, (64, 16))):
        assert exact_periods(g["tie_cur"][k]) == per == exact_periods(g["tie_prev"][k]), (k, per)
    for k in range(4):
        assert 1 in (exact_periods(g["tie_cur"][k])[0], exact_periods(g["tie_prev"][k])[0]), k  # a constant image in the pair
    assert exact_periods(g["xpow_cur"][-1]) == (64, 2) == exact_periods(g["xpow_prev"][-1])
    assert exact_periods(g["xpow_cur"][-3]) == (1, 1) and exact_periods(g["xpow_prev"][-2]) == (1, 1)
    assert exact_periods(g["bgr_cur"][-2]) == (32, 32) and exact_periods(g["bgr_cur"][-1]) == (4, 64)
    # long range: the quarter-resolution patch is the rounded mean of the 2 x 2 centre of a 4 x 4 cell of flat 2 x 2 blocks
    for k, per in ((-2, (32, 32)), (-1, (4, 64))):
        for what in ("lr_cur", "lr_prev"):
            f = g[what][k].astype(np.uint32)
            q = (f[1::4, 1::4] + f[1::4, 2::4] + f[2::4, 1::4] + f[2::4, 2::4] + 2) >> 2
            assert q.shape == (N, N) and exact_periods(q) == per, (what, k, exact_periods(q))
    assert (np.abs(g["pred"]).sum(axis=-1) > 0).all()


CASES = (("lone lane in each wave", K._gray("lone")), ("ties in one lane", K._gray("inlane")), ("two lanes of one wave", K._gray("twolanes")),
         ("several holders", K._gray("tie")), ("cross-power forms in rows 0 and 32", K._gray("xpow")), ("bgr", K._bgr),
         ("long range", K._long_range), ("window offsets gray", K._offsets(False)), ("window offsets bgr", K._offsets(True)))
