"""Inputs and CPU-oracle references of the response-gate tests (test_fft_gate_host.py, test_gpu_fft_gate.py).

Every batch mixes two classes of patches, built from the primitives of quality_cases.py: MATCHED crops of one blurred image (cur a shifted
crop of prev's image) and UNRELATED ones, where the patch of `prev` is replaced by a crop of another blurred image. The two CPU oracles
give every patch its response; test_fft_gate_host.py shows for every batch that the classes lie at least 1000 quality bars (360 d,
quality_cases.Batch.bar) apart, so no kernel within its bar can move a patch across the threshold. The threshold of a batch, `v`, is the
midpoint of that gap in the f64 oracle, and the expected gated set is the f64 oracle's !(response >= v): nothing here comes from a GPU.
Built once per process, shared, read-only."""
import functools

import numpy as np

import oracle_lib as O
import quality_cases as Q

GAP_BARS = 1000.0
FAMILY_SIZES = Q.CIRCULAR_SIZES + Q.PADDED_SIZES  # (patch size, kernel_variant) of the per-family cases
OCL_SIZES = Q.OCL_SIZES
VIDEO_SIZES = Q.VIDEO_SIZES


def unrelated(h, w, seed):
    """an h x w crop of a blurred random image that no matched pair of these batches is cut from, sigma = 2 noise"""
    return Q._noisy_u8(Q._blurred(seed + 5000, h, w), np.random.default_rng(seed + 5001))


def replace_patches(prev, n, grid, where, seed):
    """`prev` [pairs, H, W] with the n x n patch (pair, flat patch index = i + j * grid_x) of every entry of `where` replaced by an unrelated
    crop; returns the frames and the [pairs, patches] mask"""
    prev = prev.copy()
    mask = np.zeros((len(prev), grid[0] * grid[1]), bool)
    for t, (k, p) in enumerate(where):
        j, i = divmod(p, grid[0])
        prev[k, j * n:(j + 1) * n, i * n:(i + 1) * n] = unrelated(n, n, seed + 17 * t)
        mask[k, p] = True
    return prev, mask


class GateBatch:
    """A quality_cases.Batch plus the class of every patch: .unrelated [pairs, patches], .v, .gated (the f64 oracle's set) and .invalid (the
    patches the reference's validity rule already made NaN in the f64 oracle)"""

    def __init__(self, batch, mask):
        self.b, self.unrelated = batch, mask
        self.name, self.n, self.grid, self.ocl, self.cur, self.prev = batch.name, batch.n, batch.grid, batch.ocl, batch.cur, batch.prev
        r = batch.want[..., 0]
        self.lo, self.hi = float(np.nanmax(np.where(mask, r, -np.inf))), float(r[~mask].min())
        self.v = 0.5 * (self.lo + self.hi)
        self.gated = ~(r >= self.v)
        self.invalid = np.isnan(batch.shifts[..., 0])
        for a in (self.unrelated, self.gated, self.invalid):
            a.setflags(write=False)

    def gap(self, precision=64):
        """(smallest matched response, largest unrelated response) in one oracle; NaN responses (the OpenCL model's constant patch) are
        below every threshold and take no part"""
        r = (self.b.want if precision == 64 else self.b.want32)[..., 0]
        return float(r[~self.unrelated].min()), float(np.nanmax(np.where(self.unrelated, r, -np.inf)))


def _mixed_single(n, seed, ocl=False):
    """six single-patch pairs of n x n crops: even pairs matched, odd pairs against an unrelated crop"""
    cur, prev = Q.crop_pairs(n, n, 6, seed=seed)
    prev, mask = replace_patches(prev, n, (1, 1), [(1, 0), (3, 0), (5, 0)], seed)
    return GateBatch(Q.Batch(f"gate {'OpenCL model ' if ocl else ''}n={n}", n, cur, prev, ocl=ocl), mask)


@functools.lru_cache(maxsize=None)
def family(n):
    return _mixed_single(n, 7000 + n)


@functools.lru_cache(maxsize=None)
def ocl(n):
    return _mixed_single(n, 7500 + n, ocl=True)


@functools.lru_cache(maxsize=None)
def index320():
    """n = 32, an 8 x 8 grid on 256 x 256 frames, 5 pairs: 320 patches, one full workgroup of the gate kernel and a ragged one; the unrelated
    patches sit at the flat indices 0, 255, 256 and 319"""
    cur, prev = Q.crop_pairs(256, 256, 5, seed=3200)
    prev, mask = replace_patches(prev, 32, (8, 8), [divmod(f, 64) for f in (0, 255, 256, 319)], 3200)
    return GateBatch(Q.Batch("gate 8 x 8 n=32", 32, cur, prev, grid=(8, 8)), mask)


@functools.lru_cache(maxsize=None)
def grid7():
    """n = 64, a 3 x 2 grid on 192 x 128 frames, 7 pairs, one unrelated patch per pair at patch k mod 6: every (x, y) of the grid, so a
    transposed patch index gates the wrong patch"""
    cur, prev = Q.crop_pairs(128, 192, 7, seed=9700)
    prev, mask = replace_patches(prev, 64, (3, 2), [(k, k % 6) for k in range(7)], 9700)
    return GateBatch(Q.Batch("gate 3 x 2 n=64", 64, cur, prev, grid=(3, 2)), mask)


@functools.lru_cache(maxsize=None)
def video(n):
    """five frames of two patches side by side, frame 2 an unrelated image: pairs 1 and 2 are unrelated, pairs 0 and 3 matched"""
    f = Q.crop_video(n, 2 * n, 5, seed=7100 + n).copy()
    f[2] = unrelated(n, 2 * n, 7100 + n)
    g = GateBatch(Q.Batch(f"gate video n={n}", n, f[1:], f[:-1], grid=(2, 1)), np.array([[False] * 2, [True] * 2, [True] * 2, [False] * 2]))
    g.frames = f
    return g


@functools.lru_cache(maxsize=None)
def bgr64():
    """the video of video(64) as tinted BGR8 frames; the oracle sees their CV_RGB2GRAY conversion, as the kernels' loads do"""
    f = video(64).frames
    tint = np.random.default_rng(3).integers(0, 40, f.shape + (3,))
    bgr = np.clip(f[..., None].astype(np.int64) + tint, 0, 255).astype(np.uint8)
    gray = np.stack([O.rgb2gray(x) for x in bgr])
    g = GateBatch(Q.Batch("gate BGR8 video n=64", 64, gray[1:], gray[:-1], grid=(2, 1)), video(64).unrelated.copy())
    g.frames, g.bgr = gray, bgr
    return g


@functools.lru_cache(maxsize=None)
def long_range():
    """128 x 128 frames, patch size 32 (one quarter-resolution patch), four pairs, pairs 1 and 3 against an unrelated frame"""
    cur, prev = Q.crop_pairs(128, 128, 4, seed=7128, step=4)
    prev = prev.copy()
    for k in (1, 3):
        prev[k] = unrelated(128, 128, 7128 + k)
    qc, qp = np.stack([O.resize_quarter(c) for c in cur]), np.stack([O.resize_quarter(p) for p in prev])
    mask = np.array([[False], [True], [False], [True]])
    return GateBatch(Q.Batch("gate long range 128 / 32", 32, cur, prev, oracle_cur=qc, oracle_prev=qp), mask)


@functools.lru_cache(maxsize=None)
def passes200():
    """n = 200, a 2 x 1 grid, 10 pairs: four passes of three pairs through the large pipeline's scratch under MOF_FFT_LARGE_PASS=3, one gate
    launch over all of them; one unrelated patch in seven of the pairs, on either side"""
    cur, prev = Q.crop_pairs(200, 400, 10, seed=7200)
    prev, mask = replace_patches(prev, 200, (2, 1), [(0, 1), (2, 0), (3, 1), (5, 0), (6, 0), (6, 1), (9, 1)], 7200)
    return GateBatch(Q.Batch("gate passes n=200", 200, cur, prev, grid=(2, 1)), mask)


@functools.lru_cache(maxsize=None)
def rt480():
    """one 480 x 480 pair of 4 x 4 patches of 120 (the reference's default geometry), five unrelated patches: 11 valid points are left"""
    cur, prev = Q.crop_pairs(480, 480, 1, seed=4800)
    prev, mask = replace_patches(prev, 120, (4, 4), [(0, p) for p in (1, 6, 8, 11, 14)], 4800)
    return GateBatch(Q.Batch("gate getRT 480 / 120", 120, cur, prev, grid=(4, 4)), mask)


def _registry():
    r = {f"family-{n}": functools.partial(family, n) for n, _ in FAMILY_SIZES}
    r.update({f"ocl-{n}": functools.partial(ocl, n) for n, _ in OCL_SIZES})
    r.update({f"video-{n}": functools.partial(video, n) for n in VIDEO_SIZES})
    r.update({"index-320": index320, "grid-7": grid7, "bgr-64": bgr64, "long-range": long_range, "passes-200": passes200, "rt-480": rt480})
    return r


BATCHES = _registry()  # every batch test_gpu_fft_gate.py uses: name -> builder (built on first use)
