"""Inputs and CPU-oracle references of the correlation-quality tests (test_fft_quality_host.py, test_gpu_fft_quality.py).

Every batch is a list of (cur, prev) uint8 frame pairs of one geometry plus what the two CPU oracles say about it: the f64 oracle's
(response, peak) per patch -- the reference of the GPU tests -- and d, the largest distance between the f32 and the f64 oracle,
from which the GPU bar is built (360 d: the ratio of the project's shift bar, 1e-4 px, to the oracles' mutual distance on the
circular-shift pairs, 2.8e-7 px -- test_gpu_peak_tail.py). Built once per process, shared, read-only.

quality[.., 0] = response, quality[.., 1] = peak:
  cv::phaseCorrelate's model: diag.response, diag.peak_value / M^2 (M = the padded transform side)
  the OpenCL kernel's model:  diag.response, diag.peak_value, raw (its surface is already scaled)
"""
import functools

import numpy as np

import oracle_lib as O

SPEED = 1.0e4  # px: only the +-n/2 gate acts
BAR_FACTOR = 360.0
CIRCULAR_SIZES = ((32, "stockham"), (64, "stockham"), (120, "planned-half"), (54, "planned"), (200, "planned-large"))
PADDED_SIZES = ((62, "planned"), (142, "planned-half"), (196, "planned-large"))
VIDEO_SIZES = (64, 120, 128, 200)
OCL_SIZES = ((64, "stockham"), (60, "planned"), (144, "planned-large"))
# the long videos: (frame width, frames, seed, grid) -- more pairs than one run of the sequence kernels walks (runs of 2 at 64, of 4 on the
# half tile at 120 / 128 with nothing forced: mof_capi.hip fft_sequence and the launchers), a ragged last run, passes of the large video form
LONG_VIDEOS = {64: (192, 38, 6400, (3, 1)), 120: (240, 22, 12000, (2, 1)), 128: (256, 11, 12800, (2, 1)), 200: (400, 11, 20000, (2, 1))}
# long-range launches stay on the family's kernel (the planned kernel at 60, the tuned 120 kernel, L5 - L8 at 200); kernel_variant names
# the full-resolution route
LONG_RANGE_SIZES = ((60, "planned-half"), (120, "planned-half"), (200, "planned-large"))


def circular_shifts(n):
    vals = (0, 1, -1, n // 2 - 1, -(n // 2 - 1), -(n // 2))
    return [(dy, dx) for dy in vals for dx in vals]


def circular_pairs(n):
    """The 36 pairs of test_gpu_peak_tail.py: one random n x n patch (seed 7), cur = its circular shift by (dy, dx)."""
    prev = np.random.default_rng(7).integers(0, 256, (n, n), dtype=np.uint8)
    cur = np.stack([np.roll(prev, s, axis=(0, 1)) for s in circular_shifts(n)])
    return cur, np.broadcast_to(prev, cur.shape).copy()


def _blurred(seed, h, w):
    """A random image under the separable (1 6 1) / 8 blur, float64"""
    img = np.random.default_rng(seed).integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    img = (img[:-2] + 6.0 * img[1:-1] + img[2:]) / 8.0
    return (img[:, :-2] + 6.0 * img[:, 1:-1] + img[:, 2:]) / 8.0


def _noisy_u8(a, rng):
    return np.clip(np.rint(a + rng.normal(0.0, 2.0, a.shape)), 0, 255).astype(np.uint8)


def crop_pairs(h, w, count, seed, step=1):
    """`count` pairs of h x w crops of ONE blurred random image, cur shifted against prev by integers in [-8, 8] (multiples of `step`),
    sigma = 2 noise on both"""
    rng = np.random.default_rng(seed)
    base = _blurred(seed + 1000, h + 16, w + 16)
    shifts = step * rng.integers(-(8 // step), 8 // step + 1, (count, 2))
    prev = np.stack([_noisy_u8(base[8:8 + h, 8:8 + w], rng) for _ in range(count)])
    cur = np.stack([_noisy_u8(base[8 + dy:8 + dy + h, 8 + dx:8 + dx + w], rng) for dy, dx in shifts])
    return cur, prev


def crop_video(h, w, frames, seed):
    """`frames` h x w crops of one blurred random image along a walk of integer steps in [-4, 4], sigma = 2 noise on each"""
    rng = np.random.default_rng(seed)
    base = _blurred(seed + 2000, h + 8 * frames, w + 8 * frames)
    pos = 4 * frames + np.cumsum(rng.integers(-4, 5, (frames, 2)), axis=0)
    return np.stack([_noisy_u8(base[y:y + h, x:x + w], rng) for y, x in pos])


def oracle_quality(cur, prev, n, grid=(1, 1), ocl=False, precision=64):
    """[pairs, patches, 2] (response, peak), [pairs, patches] second / peak ratio, [pairs, patches, 2] shifts"""
    h, w = cur.shape[1:]
    lay = O.fft_layout(w, h, n, grid[0], grid[1], max_px_speed=SPEED)
    mm = float(O.optimal_dft_size(n)) ** 2
    q = np.empty((len(cur), grid[0] * grid[1], 2))
    ratio = np.empty(q.shape[:2])
    shifts = np.empty_like(q)
    for k in range(len(cur)):
        if ocl:
            shifts[k], _, diags = O.fft_process_ocl(cur[k], prev[k], lay, precision=precision, want_diag=True)
        else:
            shifts[k], _, diags = O.fft_process(cur[k], prev[k], lay, precision, want_diag=True)
        for p in range(q.shape[1]):
            q[k, p] = (diags[p].response, diags[p].peak_value if ocl else diags[p].peak_value / mm)
            ratio[k, p] = diags[p].second_value / diags[p].peak_value
    return q, ratio, shifts


class Batch:
    def __init__(self, name, n, cur, prev, grid=(1, 1), ocl=False, oracle_cur=None, oracle_prev=None):
        self.name, self.n, self.grid, self.ocl = name, n, grid, ocl
        self.cur, self.prev = cur, prev
        # (the long-range batch: the oracle sees the quarter-resolution frames)
        oc, op = (cur, prev) if oracle_cur is None else (oracle_cur, oracle_prev)
        self.want, self.ratio, self.shifts = oracle_quality(oc, op, n, grid, ocl, 64)
        self.want32 = oracle_quality(oc, op, n, grid, ocl, 32)[0]
        self.d_slot = np.abs(self.want32 - self.want).reshape(-1, 2).max(axis=0)  # per slot: (response, peak)
        # ONE distance per batch, the larger slot's: both slots are sums over the same f32 surface under the same scaling, and where the
        # f32 oracle happens to round a peak to the f64 value (circular shifts at n = 64, 120: 2e-11, far below an f32 ulp of the value)
        # that slot's own distance measures a coincidence, not the format
        self.d = float(self.d_slot.max())
        for a in (self.cur, self.prev, self.want, self.want32, self.ratio, self.shifts, self.d_slot):
            a.setflags(write=False)

    @property
    def bar(self):
        return BAR_FACTOR * self.d


@functools.lru_cache(maxsize=None)
def circular(n):
    cur, prev = circular_pairs(n)
    return Batch(f"circular n={n}", n, cur, prev)


@functools.lru_cache(maxsize=None)
def padded(n):
    cur, prev = crop_pairs(n, n, 12, seed=n)
    return Batch(f"padded crops n={n}", n, cur, prev)


@functools.lru_cache(maxsize=None)
def video(n):
    """a 5-frame video of two patches side by side: pair k = (frame k + 1, frame k)"""
    f = crop_video(n, 2 * n, 5, seed=n)
    b = Batch(f"video n={n}", n, f[1:], f[:-1], grid=(2, 1))
    b.frames = f
    return b


@functools.lru_cache(maxsize=None)
def crops64(count=5):
    """n = 64: the BGR8, stateful, host and graph tests share these pairs (a 2 x 2 grid of patches per frame)"""
    cur, prev = crop_pairs(128, 128, count, seed=64)
    return Batch("crops n=64", 64, cur, prev, grid=(2, 2))


@functools.lru_cache(maxsize=None)
def long_range():
    """128 x 128 frames, patch size 32: sqNum = 4, one quarter-resolution patch; shifts of whole quarter-resolution pixels (a shift that
    is no multiple of 4 does not survive the quarter resize as a shift, and the pair has no clear peak)"""
    cur, prev = crop_pairs(128, 128, 4, seed=128, step=4)
    qc, qp = np.stack([O.resize_quarter(c) for c in cur]), np.stack([O.resize_quarter(p) for p in prev])
    return Batch("long range 128 / 32", 32, cur, prev, oracle_cur=qc, oracle_prev=qp)


@functools.lru_cache(maxsize=None)
def ocl(n):
    cur, prev = crop_pairs(n, n, 12, seed=500 + n)
    return Batch(f"OpenCL model n={n}", n, cur, prev, ocl=True)


@functools.lru_cache(maxsize=None)
def grid64():
    """n = 64, 7 pairs of a NON-square grid (3 x 2): a transposed patch index, invisible on 2 x 2 only by luck, shows here; seven pairs
    make four host chunks of two with a ragged last one"""
    cur, prev = crop_pairs(128, 192, 7, seed=9600)
    return Batch("grid 3 x 2 n=64", 64, cur, prev, grid=(3, 2))


@functools.lru_cache(maxsize=None)
def passes200():
    """10 pairs of two 200-pixel patches: four passes of three pairs through the large pipeline's scratch"""
    cur, prev = crop_pairs(200, 400, 10, seed=7200)
    return Batch("passes n=200", 200, cur, prev, grid=(2, 1))


@functools.lru_cache(maxsize=None)
def ocl_passes144():
    """7 pairs of two 144-pixel patches under the OpenCL model (L5 - L8): three passes of three pairs"""
    cur, prev = crop_pairs(144, 288, 7, seed=14400)
    return Batch("OpenCL passes n=144", 144, cur, prev, grid=(2, 1), ocl=True)


@functools.lru_cache(maxsize=None)
def long_video(n):
    w, frames, seed, grid = LONG_VIDEOS[n]
    f = crop_video(n, w, frames, seed=seed)
    b = Batch(f"long video n={n}", n, f[1:], f[:-1], grid=grid)
    b.frames = f
    return b


@functools.lru_cache(maxsize=None)
def padded246():
    cur, prev = crop_pairs(246, 246, 6, seed=246)
    return Batch("padded crops n=246 (M = 250)", 246, cur, prev)


@functools.lru_cache(maxsize=None)
def crops400():
    cur, prev = crop_pairs(400, 400, 4, seed=400)
    return Batch("crops n=400", 400, cur, prev)


@functools.lru_cache(maxsize=None)
def long_range_n(n):
    """4n x 4n frames, patch size n (sqNum = 4: one quarter-resolution patch of n pixels), shifts of whole quarter-resolution pixels"""
    cur, prev = crop_pairs(4 * n, 4 * n, 4, seed=40 * n, step=4)
    qc, qp = np.stack([O.resize_quarter(c) for c in cur]), np.stack([O.resize_quarter(p) for p in prev])
    return Batch(f"long range {4 * n} / {n}", n, cur, prev, oracle_cur=qc, oracle_prev=qp)


@functools.lru_cache(maxsize=None)
def cpp_video():
    """the C++ mirror's frames (test_gpu_cpp_host.py): a 6-frame video of 128 x 128 frames, patch size 32 (a 4 x 4 grid, so the geometry
    has a long-range form)"""
    f = crop_video(128, 128, 6, seed=3200)
    b = Batch("C++ mirror video 128 / 32", 32, f[1:], f[:-1], grid=(4, 4))
    b.frames = f
    return b


SPLIT_SIZES = ((32, "stockham"), (16, "planned"), (60, "planned-half"))


@functools.lru_cache(maxsize=None)
def split_period(n):
    """Eight circular shifts of one random n x n patch along a closed walk: pair k = (shift k + 1, shift k), k mod 8 -- the period of the
    65 540-pair batches that cross a launch split of the pair kernels (the pair index rides gridDim.z, 65535 at most)"""
    base = np.random.default_rng(900 + n).integers(0, 256, (n, n), dtype=np.uint8)
    pos = np.concatenate([[(0, 0)], np.cumsum([(1, -2), (-3, 2), (0, 1), (2, 0), (1, -2), (-3, 2), (0, 1)], axis=0)])
    protos = np.stack([np.roll(base, (int(y), int(x)), axis=(0, 1)) for x, y in pos])
    b = Batch(f"split period n={n}", n, protos[(np.arange(8) + 1) % 8], protos)
    b.protos = protos
    return b


def _registry():
    r = {f"circular-{n}": functools.partial(circular, n) for n, _ in CIRCULAR_SIZES}
    r.update({f"padded-{n}": functools.partial(padded, n) for n, _ in PADDED_SIZES})
    r.update({f"video-{n}": functools.partial(video, n) for n in VIDEO_SIZES})
    r.update({"crops-64": crops64, "long-range": long_range})
    r.update({f"ocl-{n}": functools.partial(ocl, n) for n, _ in OCL_SIZES})
    r.update({"grid-64": grid64, "passes-200": passes200, "ocl-passes-144": ocl_passes144, "padded-246": padded246, "crops-400": crops400,
              "cpp-video": cpp_video})
    r.update({f"long-video-{n}": functools.partial(long_video, n) for n in LONG_VIDEOS})
    r.update({f"circular-{n}": functools.partial(circular, n) for n in (128, 250)})
    r.update({f"long-range-{n}": functools.partial(long_range_n, n) for n, _ in LONG_RANGE_SIZES})
    r.update({f"split-{n}": functools.partial(split_period, n) for n, _ in SPLIT_SIZES})
    return r


BATCHES = _registry()  # every batch test_gpu_fft_quality.py holds to the oracle: name -> builder (built on first use)
