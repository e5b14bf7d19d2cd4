"""Writes tests/golden/xpow_paths_*.npz: frame pairs (ONE n x n patch each, n = 64 and 32) that decide, bin by bin, which form of the
normalised cross-power spectrum the FFT kernels take -- C = P' rsq(q) where q = |P'|^2 >= 1024, the general form P' sqrt(q) / (q + 16 eps)
below (csrc/pc_common.hpp, cross_power_ab / cross_power_ab_batch) -- with the outputs of both oracles. Run from the repository root:

    python tests/golden/make_xpow_paths.py

  mixed      frame = 100 + 50 c[(x + y) mod 4], c = (1, 0, -1, 0): integers, so the bins (0, 0), (n/4, n/4), (3n/4, 3n/4) are large and
             every other bin of the pattern is exactly zero; one pixel raised by AMP in prev, and at the shifted place in cur
             (dx + dy = 0 mod 4), puts magnitude AMP into every bin: q = 16 AMP^4 < 1024 in n^2 - 3 bins. The lane that owns column n/4 of
             row n/4 holds one large and seven small bins.
  tile       an 8 x 8 integer tile repeated over the frame (large bins on the multiples of n/8 only) plus the same impulse: whole lanes on
             the main form beside whole lanes on the general one, in every wave.
  one_wave   the pattern and the impulse plus a weak seeded texture (synth, three bits) in rows 0..3n/4-1, the seed searched so that the few
             bins with q < 1024 all lie in the rows of ONE wave of the inverse row pass (n = 64: rows 8w .. 8w + 7 and their partners).
  main       a textured pair (synth) whose smallest q is far above 1024: the branch not taken.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
from mrs_optic_flow_amd import synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SHIFTS = ((3, 1), (6, -2), (0, 0), (-1, 5))  # (dx, dy), dx + dy = 0 (mod 4)
AMP = 2  # the raised pixel


def q_bins(cur, prev):
    """q = |P'|^2 = 16 |A|^2 |B|^2 of every bin (float64), the four real-only slots set to +inf (they take another form)."""
    a, b = np.fft.fft2(cur.astype(np.float64)), np.fft.fft2(prev.astype(np.float64))
    q = 16.0 * np.abs(a) ** 2 * np.abs(b) ** 2
    h = cur.shape[0] // 2
    for v in (0, h):
        for u in (0, h):
            q[v, u] = np.inf
    return q


def wave_of_rows(n):
    """which wave of the inverse row pass forms the bins of spectrum row v (rows 0 and n/2: wave 0's packing block, -1 here)"""
    li = 8 if n == 64 else 16
    return np.array([-1 if v in (0, n // 2) else min(v, n - v) // li for v in range(n)])


def pattern(n):
    y, x = np.mgrid[0:n, 0:n]
    return 100 + 50 * np.array([1, 0, -1, 0])[(x + y) % 4]


def impulse_pair(base, n, dx, dy, amp):
    py, px = (20, 27) if n == 64 else (10, 13)
    prev, cur = base.copy(), base.copy()
    prev[py, px] += amp
    cur[py + dy, px + dx] += amp
    return cur, prev


def texture_rows(n, k):
    """three bits of the seeded canvas in rows 0 .. 3n/4 - 1 (not shifted between the frames: the impulse carries the shift)"""
    t = (synth.canvas_np(k, n, n, blur=False)[:n, :n] >> 5).astype(np.int64)
    t[3 * n // 4:] = 0
    return t


def build(n):
    out = {}
    base = pattern(n)
    out["mixed"] = [impulse_pair(base, n, dx, dy, AMP) for dx, dy in SHIFTS]
    tile = (synth.canvas_np(5, 8, 8, blur=False)[:8, :8] >> 1).astype(np.int64) + 60
    out["tile"] = [impulse_pair(np.tile(tile, (n // 8, n // 8)), n, dx, dy, AMP) for dx, dy in SHIFTS]
    waves = wave_of_rows(n)
    found = []
    for k in range(4000):
        cur, prev = impulse_pair(base + texture_rows(n, k), n, *SHIFTS[len(found)], AMP)
        q = q_bins(cur, prev)
        rare_rows = np.unique(np.nonzero(q < 1024.0)[0])
        w = set(waves[rare_rows])
        # (a margin around the threshold: the kernel's q is an f32 number from the packed transform)
        if len(rare_rows) and len(w) == 1 and -1 not in w and not ((q > 512.0) & (q < 2048.0)).any() and (n == 32 or next(iter(w)) == len(found)):  # (n = 64: pair i -> wave i)
            found.append((cur, prev, k, next(iter(w))))
            if len(found) == len(SHIFTS):
                break
    assert len(found) == len(SHIFTS), (n, len(found))
    out["one_wave"] = [(c, p) for c, p, _, _ in found]
    print(f"n = {n}: one_wave seeds {[(k, w) for _, _, k, w in found]}")
    main = []
    k = 0
    while len(main) < len(SHIFTS):
        dx, dy = SHIFTS[len(main)]
        cur, prev = synth.pair_np(300 + k, n, n, dx, dy)
        k += 1
        if q_bins(cur, prev).min() >= 65536.0:
            main.append((cur, prev))
    out["main"] = main
    return out


def main():
    for n in (64, 32):
        lay = O.fft_layout(n, n, n, 1, 1)
        for name, pairs in build(n).items():
            cur, prev = np.stack([c for c, _ in pairs]), np.stack([p for _, p in pairs])
            assert min(cur.min(), prev.min()) >= 0 and max(cur.max(), prev.max()) <= 255
            cur, prev = cur.astype(np.uint8), prev.astype(np.uint8)
            w64 = np.stack([O.fft_process(cur[i], prev[i], lay, 64)[0] for i in range(len(pairs))])
            w32 = np.stack([O.fft_process(cur[i], prev[i], lay, 32)[0] for i in range(len(pairs))])
            q = np.stack([q_bins(cur[i], prev[i]) for i in range(len(pairs))])
            print(f"n = {n} {name}: bins below 1024 {[int((x < 1024.0).sum()) for x in q]}, smallest q {[float(x.min()) for x in q]}\n"
                  f"    f64 oracle {w64[:, 0].tolist()}\n    f32 - f64 {np.abs(w32 - w64).max():.3g} px")
            np.savez_compressed(os.path.join(HERE, f"xpow_paths_{name}_n{n}.npz"), n=n, cur=cur, prev=prev, oracle64=w64, oracle32=w32,
                                shifts=np.array(SHIFTS))


if __name__ == "__main__":
    main()
