"""Inputs and CPU-oracle references of the launch-form tests (test_gpu_fft_launch_forms.py; the knob children of
test_gpu_fft_quality_forms.py; the bit corpus of tools/tail_bits.py).

One case = one front-end FORM of one launcher of csrc/: (gray | BGR8 | long-range) x (cv::phaseCorrelate's | the OpenCL kernel's peak
model) on a few frame pairs -- or a 3-frame video -- of a few patches from mrs_optic_flow_amd.synth (the "mild" blur, planted integer
shifts). A launcher that picks the WRONG form on these bytes must fail, not pass by accident, so the inputs are built to tell the
forms apart (`neighbours`, checked on the CPU by `assert_forms_apart` before a GPU is touched):
  - the other peak model on the same bytes (where the reference has that model at the size: an even size that is not padded);
  - BGR8 bytes read as a gray frame -- the plane of the first channel, and the bytes as they lie (the first W bytes of each row of
    3 W) --: the first channel carries another texture under another shift than the two that dominate CV_RGB2GRAY.
Everything is built on first use, cached, and read-only."""
import functools

import numpy as np

import oracle_lib as O
import tolerances as T
from mrs_optic_flow_amd import synth

SPEED = 1.0e4  # px: only the +-n/2 gate acts
M = synth.MARGIN


def _planted(k, n):
    """the planted (dx, dy) of pair k and the first BGR8 channel's, two pixels away in both axes; both stay below n / 2"""
    s = max(1, min(5, n // 4 - 1))
    dx, dy = synth.planted_shift(k, s)
    return (dx, dy), (dx - 2 if dx > 0 else dx + 2, dy - 2 if dy > 0 else dy + 2)


def _window(k, h, w, ox, oy):
    """the h x w window of texture k whose content sits (ox, oy) pixels from where the window at (0, 0) shows it"""
    c = synth.canvas_np(k, h, w, "mild")
    return c[M - oy:M - oy + h, M - ox:M - ox + w]


class Case:
    """kind 'pairs': self.cur, self.prev [pairs, H, W(, 3)]; kind 'video': self.frames [frames, H, W(, 3)], pair k = (frame k + 1, frame k)"""

    def __init__(self, name, n, variant, channels=1, ocl=False, long_range=False, kind="pairs", grid=(2, 2), count=2, seed=0):
        self.name, self.n, self.variant, self.channels, self.ocl, self.long_range, self.kind = name, n, variant, channels, ocl, long_range, kind
        self.count, self.seed = count, seed
        self.grid = (1, 1) if long_range else grid            # patches the kernels see
        f = 4 if long_range else 1                            # frame pixels per pixel the kernels transform
        self.shape = (4 * n, 4 * n) if long_range else (grid[1] * n, grid[0] * n)
        self.scale = f

    # ---- the bytes the entries receive --------------------------------------------------------------------------------------------
    @functools.cached_property
    def _offsets(self):
        """per frame of the video (or per (prev, cur) of each pair): the content's offsets, main texture and first BGR8 channel"""
        if self.kind == "video":
            main, first = [(0, 0)], [(0, 0)]
            for k in range(self.count - 1):
                d, d0 = _planted(self.seed + k + 1, self.n)
                main.append((main[-1][0] + d[0], main[-1][1] + d[1]))
                first.append((first[-1][0] + d0[0], first[-1][1] + d0[1]))
            return main, first
        return None

    def _frame(self, k, off, off0):
        h, w = self.shape
        f = self.scale
        g = _window(self.seed + k, h, w, f * off[0], f * off[1])
        if self.channels == 1:
            return g
        return np.stack([_window(self.seed + k + 200, h, w, f * off0[0], f * off0[1]), g, _window(self.seed + k + 100, h, w, f * off[0], f * off[1])], axis=-1)

    @functools.cached_property
    def frames(self):
        assert self.kind == "video"
        main, first = self._offsets
        a = np.stack([self._frame(0, main[t], first[t]) for t in range(self.count)])  # (one texture: the video walks over it)
        a.setflags(write=False)
        return a

    @functools.cached_property
    def _pairs(self):
        if self.kind == "video":
            return self.frames[1:], self.frames[:-1]
        cur, prev = [], []
        for k in range(self.count):
            d, d0 = _planted(self.seed + k + 1, self.n)
            cur.append(self._frame(k, d, d0))
            prev.append(self._frame(k, (0, 0), (0, 0)))
        cur, prev = np.stack(cur), np.stack(prev)
        cur.setflags(write=False)
        prev.setflags(write=False)
        return cur, prev

    cur = property(lambda self: self._pairs[0])
    prev = property(lambda self: self._pairs[1])

    # ---- what the oracles say -----------------------------------------------------------------------------------------------------
    def _oracle(self, cur, prev, ocl, precision):
        """[pairs, patches, 2] shifts of gray frame pairs under this case's geometry (long range: on the oracle's quarter resize)"""
        if self.long_range:
            cur, prev = np.stack([O.resize_quarter(c) for c in cur]), np.stack([O.resize_quarter(p) for p in prev])
        h, w = cur.shape[1:]
        lay = O.fft_layout(w, h, self.n, self.grid[0], self.grid[1], max_px_speed=SPEED)
        run = (lambda c, p: O.fft_process_ocl(c, p, lay, precision=precision)[0]) if ocl else (lambda c, p: O.fft_process(c, p, lay, precision)[0])
        return np.stack([run(np.ascontiguousarray(c), np.ascontiguousarray(p)) for c, p in zip(cur, prev)])

    def _gray(self, a):
        return a if self.channels == 1 else np.stack([O.rgb2gray(f) for f in a])

    @functools.cached_property
    def gray(self):
        """(cur, prev) as the right form sees them before any resize"""
        return self._gray(self.cur), self._gray(self.prev)

    @functools.cached_property
    def want(self):
        """(f64 oracle, f32 oracle) [pairs, patches, 2]"""
        w64, w32 = (self._oracle(*self.gray, self.ocl, p) for p in (64, 32))
        w64.setflags(write=False)
        w32.setflags(write=False)
        return w64, w32

    @property
    def has_other_model(self):
        return self.n % 2 == 0 and O.optimal_dft_size(self.n) == self.n

    @functools.cached_property
    def neighbours(self):
        """{what: f64 oracle's shifts of the neighbouring form on the same bytes}"""
        out = {}
        if self.has_other_model:
            out["the other peak model"] = self._oracle(*self.gray, not self.ocl, 64)
        if self.channels == 3:
            w = self.shape[1]
            out["the first channel as a gray frame"] = self._oracle(self.cur[..., 0], self.prev[..., 0], self.ocl, 64)
            out["the BGR8 bytes as a gray frame"] = self._oracle(self.cur.reshape(self.cur.shape[0], -1, 3 * w)[..., :w],
                                                                 self.prev.reshape(self.prev.shape[0], -1, 3 * w)[..., :w], self.ocl, 64)
        return out


def assert_forms_apart(case):
    """On at least half of the case's patches every neighbouring form's answer is more than two bars from the expected one -- a kernel
    within one bar of a wrong form's answer is then more than one bar from the right one. The bar of a patch is never above
    tolerances.CEILING (check_patch), so two ceilings stand for two bars of any patch. Returns {what: patches apart} for the test's print."""
    want = case.want[0]
    apart = {}
    for what, other in case.neighbours.items():
        far = (np.isnan(other) != np.isnan(want)).any(axis=-1) | (np.nan_to_num(np.abs(other - want)).max(axis=-1) > 2 * T.CEILING)
        apart[what] = int(far.sum())
        assert 2 * apart[what] >= far.size, (case.name, what, apart[what], far.size, want.tolist(), other.tolist())
    return apart


def engine(case):
    from mrs_optic_flow_amd import FftMethod
    from mrs_optic_flow_amd.engine import PEAK_OCL

    pk = PEAK_OCL if case.ocl else 0
    if case.long_range:
        return FftMethod(4 * case.n, case.n, SPEED, peak_model=pk)
    return FftMethod(sample_point_size=case.n, max_px_speed=SPEED, frame_shape=case.shape, grid=case.grid, peak_model=pk)


def run(case, fm, dev, return_quality=False):
    """the case through the public entry that expresses its form; a tensor [pairs, patches, 2] (with return_quality: shifts, quality)"""
    import torch

    def gpu(a):
        return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared inputs are read-only)

    if case.kind == "video":
        entry = fm.process_sequence_device_bgr if case.channels == 3 else fm.process_sequence_device
        return entry(gpu(case.frames), return_quality=return_quality)
    entry = fm.process_long_range_batch_device if case.long_range else (fm.process_batch_device_bgr if case.channels == 3 else fm.process_batch_device)
    return entry(gpu(case.cur), gpu(case.prev), return_quality=return_quality)


def check(case, got, what):
    """Every patch of the case through tests/tolerances.py's check_patch (a patch off its fast path is classified from its pixels and
    recorded there, as everywhere); returns the number pinned"""
    w64, w32 = case.want
    gc, gp = case.gray
    if case.long_range:
        gc, gp = np.stack([O.resize_quarter(c) for c in gc]), np.stack([O.resize_quarter(p) for p in gp])
    lay = O.fft_layout(gc.shape[2], gc.shape[1], case.n, case.grid[0], case.grid[1], max_px_speed=SPEED)
    assert got.shape == w64.shape and got.dtype == np.float64, (case.name, got.shape, w64.shape)
    return sum(bool(T.check_patch(got[k, p], w64[k, p], w32[k, p], f"launch form {case.name}/pair {k}", p, what=what,
                                  pixels=T.patch_pixels(gc[k], gp[k], lay, p)))
               for k in range(got.shape[0]) for p in range(got.shape[1]))


def _cases():
    out = []

    def add(name, n, variant, **kw):
        out.append(Case(name, n, variant, seed=1000 * len(out) + n, **kw))

    fronts = (("gray", 1), ("bgr", 3))
    models = (("cv", False), ("ocl", True))
    # K1 (pc_kernel.hip at 32 / 64 / 128; 120: the half-tile kernel under cv::phaseCorrelate's model, pc_kernel_mixed.hip under the OpenCL
    # model and in the long-range mode): 2 pairs of a 2 x 2 grid, one 4n x 4n pair in the long-range mode
    for n in (32, 64, 120, 128):
        for mname, ocl in models:
            variant = "planned-half" if (n == 120 and not ocl) else "stockham"
            for fname, ch in fronts:
                add(f"k1-{n}-{fname}-{mname}", n, variant, channels=ch, ocl=ocl)
            add(f"k1-{n}-lr-{mname}", n, variant, ocl=ocl, long_range=True, count=1)
    # the planned kernel (pc_kernel_generic.hip): 11 -> 12 (the run-time plan: below 16), 20 (the smallest compile-time plan), 74 -> 75
    # (an odd padded size). The reference has the OpenCL model at 20 only (11 and 74 are padded).
    for n in (11, 20, 74):
        for mname, ocl in models if n == 20 else models[:1]:
            for fname, ch in fronts:
                add(f"planned-{n}-{fname}-{mname}", n, "planned", channels=ch, ocl=ocl)
            add(f"planned-{n}-lr-{mname}", n, "planned", ocl=ocl, long_range=True, count=1)
    # the half-tile kernel (pc_half_kernel.hip)
    for n in (60, 144):
        for fname, ch in fronts:
            add(f"half-{n}-{fname}", n, "planned-half", channels=ch)
    # the large pipeline's rows (pc_large_kernel.hip, L5): the OpenCL model at 144 -- the smallest size beyond a CU's tile that the
    # reference plans under that model (136 = 8 x 17 has no plan) --, the long-range mode at 200
    for fname, ch in fronts:
        add(f"large-144-{fname}-ocl", 144, "planned-large", channels=ch, ocl=True, grid=(2, 1))
    add("large-200-lr", 200, "planned-large", long_range=True, count=1)
    # the video entry: pc_seq_kernel's four forms (64), pc_seq_half_kernel<128, 1, .> (the OpenCL model at 128) and the half-tile
    # kernel's video form (128, 50, 120 under cv::phaseCorrelate's model); 3 frames
    for n in (64, 128):
        for mname, ocl in models:
            for fname, ch in fronts:
                add(f"video-{n}-{fname}-{mname}", n, "stockham", channels=ch, ocl=ocl, kind="video", count=3)
    for n, variant in ((50, "planned"), (120, "planned-half")):
        for fname, ch in fronts:
            add(f"video-{n}-{fname}-cv", n, variant, channels=ch, kind="video", count=3)
    return {c.name: c for c in out}


CASES = _cases()  # name -> Case, the forms of the DEFAULT route; the knob children pick theirs by name (MOF_LAUNCH_FORM_CASES)
