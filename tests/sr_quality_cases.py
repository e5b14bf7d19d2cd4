"""Inputs and CPU-oracle references of the estimator's correlation-quality tests (test_sr_quality_host.py, test_gpu_sr_quality.py).

The reference is assembled from the unchanged oracle's pieces: O.logpolar gives the log-polar images (INTER_CUBIC for the first frame
of an estimator, INTER_LANCZOS4 for every later one -- scaleRotationEstimator.cpp:45, :112), O.phase_correlate(cur_lp, prev_lp, 64) gives
pt and the surface's `response` and `peak_value`, and `Machine` is scaleRotationEstimator::processImage's state machine (:34-148) around
them with both gates: the reference's |pt.x| > resolution / 2 and the response gate of include/mof.h. With min_response = 0 it IS
O.ScaleRotationEstimator (test_sr_quality_host.py holds it to that, exactly).

quality[.., 0] = response, quality[.., 1] = peak_value / M^2, M = getOptimalDFTSize(resolution); (NaN, NaN) where no correlation ran.
d = the largest distance between the f32 and the f64 oracle over both slots of a batch; the GPU bar is quality_cases.BAR_FACTOR * d, the
rule of the FFT engine's quality tests. Built once per process, shared, read-only.
"""
import functools
import math

import numpy as np

import oracle_lib as O
import sr_scenes
from quality_cases import BAR_FACTOR

INTER_CUBIC, INTER_LANCZOS4 = 2, 4
# the five views of test_gpu_generic.py::test_scale_rotation_at_any_resolution, of sr_scenes.canvas(11 + res, res)
VIEW_PARAMS = ((1.0, 0.0), (1.03, 2.0), (0.96, -3.0), (1.0, 5.0), (1.05, -1.0))
# the smallest resolution on each route of mof_sr.hip's sr_route
ROUTES = ((100, 22.0), (104, 22.0), (250, 40.0), (144, 28.0), (240, 40.0))
ROUTE_NOTES = {100: "tuned transforms, K8", 104: "pads to 108: K5s / K6s / K7 + L8", 250: "the exact-sums form + L8",
               144: "the route test_scale_rotation_at_any_resolution names for 144", 240: "always tuned"}
GATE_CASES = ((100, 22.0), (144, 28.0))
MIN_RESPONSE = 0.4
NOISE_AT = 3  # the gate video: [v0, v1, v2, noise(seed 5), v3, v4]


@functools.lru_cache(maxsize=None)
def views(res):
    base = sr_scenes.canvas(11 + res, res)
    v = np.stack([sr_scenes.view(base, res, s, r) for s, r in VIEW_PARAMS])
    v.setflags(write=False)
    return v


def noise(res, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (res, res), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def gate_video(res):
    v = views(res)
    f = np.stack([v[0], v[1], v[2], noise(res), v[3], v[4]])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference_gate_video():
    """12 frames of uniform noise at 100^2, M = 22: frame 6 fails the reference's rule (|pt.x| > 50 in the oracle), so frame 7 is
    correlated with frame 5"""
    f = np.random.default_rng(6).integers(0, 256, (12, 100, 100), dtype=np.uint8)
    f.setflags(write=False)
    return f


def correlate(cur_lp, prev_lp):
    """pt, f64 quality, f32 quality of cv::phaseCorrelate(cur_lp, prev_lp)"""
    mm = float(O.optimal_dft_size(cur_lp.shape[0])) ** 2
    pt, d64 = O.phase_correlate(cur_lp, prev_lp, 64)
    _, d32 = O.phase_correlate(cur_lp, prev_lp, 32)
    return pt, np.array([d64["response"], d64["peak_value"] / mm]), np.array([d32["response"], d32["peak_value"] / mm])


class Machine:
    """processImage with both gates. step(frame) -> (out[4] = scale, rot, pt.x, pt.y; quality[2]; f32 oracle's quality[2]; gated)"""

    def __init__(self, res, M, min_response=0.0, variant=0):
        self.res, self.M, self.min_response, self.variant = res, float(M), float(min_response), variant
        self.prev_lp = None

    def step(self, frame):
        nan2 = np.full(2, np.nan)
        if self.prev_lp is None:  # :36-74
            self.prev_lp = O.logpolar(frame, self.M, INTER_CUBIC, variant=self.variant)
            return np.array([1.0, 0.0, 0.0, 0.0]), nan2, nan2, False
        lp = O.logpolar(frame, self.M, INTER_LANCZOS4, variant=self.variant)  # (transparent pixels stay the zeros tempIm started with)
        pt, q, q32 = correlate(lp, self.prev_lp)
        gated = abs(pt[0]) > self.res // 2 or (self.min_response > 0.0 and not q[0] >= self.min_response)
        if gated:  # :119-121: (1, 0), the previous image stays
            return np.array([1.0, 0.0, pt[0], pt[1]]), q, q32, True
        self.prev_lp = lp  # :128
        ky = self.res / 360.0
        return np.array([math.exp(pt[0] / self.M), (pt[1] / ky) * (3.14159265358979323846 / 180), pt[0], pt[1]]), q, q32, False


class Ref:
    def __init__(self, name, steps):
        self.name = name
        self.out = np.stack([s[0] for s in steps])
        self.quality = np.stack([s[1] for s in steps])
        self.quality32 = np.stack([s[2] for s in steps])
        self.gated = np.array([s[3] for s in steps])
        ran = ~np.isnan(self.quality[:, 0])
        self.d = float(np.abs(self.quality32[ran] - self.quality[ran]).max())
        for a in (self.out, self.quality, self.quality32, self.gated):
            a.setflags(write=False)

    @property
    def bar(self):
        return BAR_FACTOR * self.d


def run_video(frames, res, M, min_response=0.0, variant=0, name="video"):
    """the frames through ONE machine: what the stateful loop and the resolved sequence entry compute"""
    m = Machine(res, M, min_response, variant)
    ref = Ref(name, [m.step(f) for f in frames])
    ref.machine = m  # (left in the state after the last frame)
    return ref


def run_pairs(cur, prev, res, M, min_response=0.0, variant=0, name="pairs"):
    """every pair the two-call sequence of a fresh machine fed (prev, cur): what the batch entry computes"""
    steps = []
    for c, p in zip(cur, prev):
        m = Machine(res, M, min_response, variant)
        m.step(p)
        steps.append(m.step(c))
    return Ref(name, steps)


def run_consecutive(frames, res, M, min_response=0.0, name="consecutive"):
    """the asynchronous sequence entry: the output is gated, every frame is correlated with its immediate predecessor"""
    steps = []
    for k, f in enumerate(frames):
        m = Machine(res, M, min_response)
        if k > 0:
            m.prev_lp = O.logpolar(frames[k - 1], M, INTER_CUBIC if k == 1 else INTER_LANCZOS4)
        steps.append(m.step(f))
    return Ref(name, steps)


@functools.lru_cache(maxsize=None)
def route_video(res, M, variant=0):
    return run_video(views(res), res, M, variant=variant, name=f"views {res} / {M}: video")


@functools.lru_cache(maxsize=None)
def route_pairs(res, M, variant=0):
    v = views(res)
    return run_pairs(v[1:], v[:-1], res, M, variant=variant, name=f"views {res} / {M}: pairs")


@functools.lru_cache(maxsize=None)
def gate_refs(res, M):
    """the gate video of (res, M) under MIN_RESPONSE: resolved, asynchronous, as pairs -- and resolved with the gate off"""
    f = gate_video(res)
    return dict(video=run_video(f, res, M, MIN_RESPONSE, name=f"gate video {res}"),
                consecutive=run_consecutive(f, res, M, MIN_RESPONSE, name=f"gate video {res}, consecutive"),
                pairs=run_pairs(f[1:], f[:-1], res, M, MIN_RESPONSE, name=f"gate video {res}, pairs"),
                off=run_video(f, res, M, 0.0, name=f"gate video {res}, gate off"))
