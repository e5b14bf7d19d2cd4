#!/usr/bin/env python3
"""Latency of the node's own call pattern, one host frame in, a host result out: FftMethod.processImage on the reference default geometry
(480 x 480 crop, 4 x 4 patches of 120 x 120), c2's and three planned sizes; FastSpacedBMMethod.processBlocks (mof_bm_process_q) at c3's
geometry; scaleRotationEstimator.processImage (mof_sr_process) at 480 x 480.
usage (GPU box): python tools/stateful_latency.py [--tree DIR] [substring of a case name ...]
  --tree DIR: the package of another checkout (tools/ab_commit.sh prepare puts the parent's at tmp_ab/parent), for A/B runs of this file's cases"""
import os, sys, time
args = sys.argv[1:]
tree = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if args[:1] == ["--tree"]:
    tree, args = os.path.abspath(args[1]), args[2:]
sys.path.insert(0, tree)
import numpy as np
from mrs_optic_flow_amd import FastSpacedBMMethod, FftMethod, ScaleRotationEstimator, synth


def fft(*a, **kw):
    fm = FftMethod(*a, **kw)
    return fm.processImage


CASES = (("ref 480^2, 4x4 x 120^2", lambda: fft(480, 120, 80.0), (480, 480)),
         ("c2 752x480, 8x8 x 64^2", lambda: fft(sample_point_size=64, frame_shape=(480, 752), grid=(8, 8), origin=(1, 1), stride=(98, 59)), (480, 752)),
         # r04: a size without a tuned kernel (the planned kernel), and the reference's whole-frame fallback (470 / 100 does not
         # divide: ONE 470 x 470 patch, padded to 480 -- the planned pipeline; 480 / 100: one 480 x 480 patch -- the estimator's kernels)
         ("480^2, 8x8 x 60^2 (planned)", lambda: fft(480, 60, 80.0), (480, 480)),
         ("470^2 / 100 -> one 470^2 patch (planned-large)", lambda: fft(470, 100, 80.0), (470, 470)),
         ("480^2 / 100 -> one 480^2 patch (tuned transforms)", lambda: fft(480, 100, 80.0), (480, 480)),
         # the stateful calls of the other two engines: one scan + mode launch, one remap + three transform launches
         ("bm c3 752x480, 16^2 step 8 radius 16 (scan16)", lambda: FastSpacedBMMethod(16, 16, 8, (480, 752)).processBlocks, (480, 752)),
         ("sr 480^2, M 49.9", lambda: ScaleRotationEstimator(480, 49.9).processImage, (480, 480)))

for name, make, shape in CASES:
    if args and not any(a in name for a in args):
        continue
    call = make()
    frames = [synth.pair_np(5 + t, shape[0], shape[1], t % 5, -(t % 3))[0] for t in range(8)]
    for f in frames[:3]:
        call(f)
    ts = []
    for t in range(200):
        f = frames[t % 8]
        t0 = time.perf_counter()
        call(f)
        ts.append(time.perf_counter() - t0)
    ts = np.sort(np.array(ts)) * 1e3
    print(f"{name}: one call (host frame) median {ts[100]:.3f} ms, p90 {ts[180]:.3f} ms, min {ts[0]:.3f} ms")
