"""Writes tests/golden/argmax_paths_n{64,32}.npz: frame pairs (ONE n x n patch each) that put the first maximum of the correlation
surface into every part of K1's arg-max -- each wave's column range, both packed halves (columns below and above n/2), every row residue
of the last column stage -- and pairs whose surface attains its maximum more than once. Run from the repository root:

    python tests/golden/make_argmax_paths.py           the inputs and the oracle's peaks (no GPU)
    python tests/golden/make_argmax_paths.py record    adds what the library computes for them on the GPU: run ONCE, with the build the
                                                       arg-max is to be held to (the commit before the value-first arg-max)

  sweep     prev = a random u8 texture, cur = prev rolled by (dy, dx): the surface is one sharp sample at the planted shift.
            n = 64: dx in DX64 x dy in DY64 (the shifted column n/2 + dx walks through the four waves' columns and both halves of a
            packed pair, the shifted row n/2 + dy through every residue mod 8); n = 32: the analogous set.
  periodic  textures of period p in x, in y and in both, cur == prev and cur rolled by a multiple of p: the surface repeats with that
            period, so equal or nearly equal maxima sit in one lane, in several lanes and in several waves.
  constant  one constant pair and one pair with a constant prev (the degenerate substitute of the tail).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HERE = os.path.dirname(os.path.abspath(__file__))
DX = {64: (-32, -25, -17, -9, -1, 0, 7, 15, 23, 31), 32: (-16, -13, -9, -5, -1, 0, 3, 7, 11, 15)}
DY = {64: (-32, -27, -18, -9, 0, 5, 14, 23, 31), 32: (-16, -14, -9, -5, 0, 2, 7, 11, 15)}
PERIODS = {64: (8, 16, 32), 32: (4, 8, 16)}


def texture(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, n), dtype=np.uint8)


def build(n):
    """-> list of (name, cur, prev, planted (dx, dy) or None where the surface has no single sharp maximum)"""
    cases = []
    prev = texture(n, 1000 + n)
    for dy in DY[n]:
        for dx in DX[n]:
            cases.append((f"sweep dx={dx} dy={dy}", np.roll(prev, (dy, dx), axis=(0, 1)), prev, (dx, dy)))
    for p in PERIODS[n]:
        t = texture(p, 2000 + n + p)
        for axes, tile in (("x", np.tile(texture(n, 3000 + n + p)[:, :p], (1, n // p))),
                           ("y", np.tile(texture(n, 4000 + n + p)[:p, :], (n // p, 1))),
                           ("xy", np.tile(t, (n // p, n // p)))):
            cases.append((f"period {p} {axes} same", tile.copy(), tile, None))
            roll = (p if "y" in axes else 0, 2 * p % n if "x" in axes else 0)
            cases.append((f"period {p} {axes} rolled", np.roll(tile, roll, axis=(0, 1)), tile, None))
    cases.append(("constant pair", np.full((n, n), 77, np.uint8), np.full((n, n), 77, np.uint8), None))
    cases.append(("constant prev", texture(n, 5000 + n), np.full((n, n), 130, np.uint8), None))
    return cases


def path(n):
    return os.path.join(HERE, f"argmax_paths_n{n}.npz")


def main():
    import oracle_lib as O

    for n in (64, 32):
        cases = build(n)
        cur, prev = np.stack([c for _, c, _, _ in cases]), np.stack([p for _, _, p, _ in cases])
        planted = np.array([s if s is not None else (np.nan, np.nan) for _, _, _, s in cases], np.float64)
        peaks = np.array([O.phase_correlate(cur[k], prev[k], 64)[1]["peak"] for k in range(len(cases))], np.float64)
        np.savez_compressed(path(n), n=n, names=np.array([c[0] for c in cases]), cur=cur, prev=prev, planted=planted, oracle_peak=peaks)
        print(f"n = {n}: {len(cases)} pairs, {os.path.getsize(path(n))} bytes")


def record():
    """what the library in use computes, through the default entry and the _q entry; bits are kept (float64 arrays)"""
    import torch

    from mrs_optic_flow_amd import FftMethod

    for n in (64, 32):
        g = dict(np.load(path(n)))
        fm = FftMethod(sample_point_size=n, frame_shape=(n, n), grid=(1, 1))
        tc, tp = torch.from_numpy(g["cur"]).cuda(), torch.from_numpy(g["prev"]).cuda()
        g["want_shift"] = fm.process_batch_device(tc, tp).cpu().numpy()[:, 0]
        s, q = fm.process_batch_device(tc, tp, return_quality=True)
        g["want_shift_q"], g["want_quality"] = s.cpu().numpy()[:, 0], q.cpu().numpy()[:, 0]
        np.savez_compressed(path(n), **g)
        print(f"n = {n}: recorded {len(g['want_shift'])} pairs; NaN shifts {int(np.isnan(g['want_shift'][:, 0]).sum())}; "
              f"default == _q bits {np.array_equal(g['want_shift'].view(np.uint64), g['want_shift_q'].view(np.uint64))}")


if __name__ == "__main__":
    record() if sys.argv[1:] == ["record"] else main()
