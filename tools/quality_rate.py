#!/usr/bin/env python3
"""What the per-patch quality output (include/mof.h, the *_q entries; return_quality=True) costs: pairs/s of the FFT engine with and
without it at bench.py's geometries c2, ref, c4, l200 (pair entry) and c2seq (video entry), and of the scale / rotation estimator at c5
(pair entry) and c5seq (video entry, asynchronous as bench.py runs it) -- quoted in README.md, profiles/quality_ab.txt and
profiles/sr_quality.txt; never bench.py's `value`.
usage (GPU box): python tools/quality_rate.py [reps] [workload ...]    -> one JSON line per workload

Both forms run on the same frames into preallocated-size outputs, alternating call by call, each call timed with device events; the
rate is pairs / median. `shifts_same_bits` confirms that the shifts do not depend on the quality pointer."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mrs_optic_flow_amd import FftMethod, ScaleRotationEstimator, synth

# bench.py's geometries (WORKLOADS); batch = frame pairs per call
WORKLOADS = {
    "c2": dict(h=480, w=752, n=64, grid=(8, 8), origin=(1, 1), stride=(98, 59), batch=1024, video=False),
    "ref": dict(h=480, w=480, n=120, grid=(4, 4), origin=(0, 0), stride=(120, 120), batch=1024, video=False),
    "c4": dict(h=1080, w=1920, n=128, grid=(16, 16), origin=(0, 0), stride=(119, 63), batch=256, video=False),
    "l200": dict(h=480, w=480, n=200, grid=(2, 2), origin=(0, 0), stride=(200, 200), batch=512, video=False),
    "c2seq": dict(h=480, w=752, n=64, grid=(8, 8), origin=(1, 1), stride=(98, 59), batch=1024, video=True),
    # the estimator's share of c5 / c5seq: the 480 x 480 centre crop of the 752-wide frames, M = 49.9, 1024-pair passes
    "c5": dict(h=480, w=752, sr_res=480, sr_m=49.9, batch=1024, video=False),
    "c5seq": dict(h=480, w=752, sr_res=480, sr_m=49.9, batch=1024, video=True),
}
args = sys.argv[1:]
REPS = max(10, int(args[0])) if args and args[0].isdigit() else 20
names = [a for a in args if not a.isdigit()] or list(WORKLOADS)
dev = torch.device("cuda:0")


def timed_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


for name in names:
    w = WORKLOADS[name]
    B = w["batch"]
    video, _ = synth.video_torch(B + 1, w["h"], w["w"], dev, k=1)
    if "sr_res" in w:
        r = w["sr_res"]
        x0 = (w["w"] - r) // 2
        crop = video[:, :r, x0:x0 + r]
        fm = ScaleRotationEstimator(r, w["sr_m"], batch_chunk=1024)
        fm.process_sequence_device(crop[:2])  # armed: every timed frame goes through INTER_LANCZOS4
        fm.kernel_variant, fm.n_patches = "estimator", 1
        if w["video"]:
            off = lambda: fm.process_sequence_device(crop[1:], resolve_gate=False)
            on = lambda: fm.process_sequence_device(crop[1:], resolve_gate=False, return_quality=True)
        else:
            off = lambda: fm.process_batch_device(crop[1:], crop[:-1])
            on = lambda: fm.process_batch_device(crop[1:], crop[:-1], return_quality=True)
    else:
        fm = FftMethod(sample_point_size=w["n"], frame_shape=(w["h"], w["w"]), grid=w["grid"], origin=w["origin"], stride=w["stride"])
        if w["video"]:
            off = lambda: fm.process_sequence_device(video)
            on = lambda: fm.process_sequence_device(video, return_quality=True)
        else:
            off = lambda: fm.process_batch_device(video[1:], video[:-1])
            on = lambda: fm.process_batch_device(video[1:], video[:-1], return_quality=True)
    for _ in range(3):
        off()
        on()
    t_off, t_on = [], []
    for _ in range(REPS):  # alternating
        ms, plain = timed_ms(off)
        t_off.append(ms)
        ms, (shifts, quality) = timed_ms(on)
        t_on.append(ms)
    torch.cuda.synchronize()
    same = bool(torch.equal(plain.view(torch.int64), shifts.view(torch.int64)))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    print(json.dumps(dict(workload=name, kernel_variant=fm.kernel_variant, pairs=B, patches=fm.n_patches, reps=REPS,
                          off_ms=round(m_off, 4), on_ms=round(m_on, 4), off_pairs_per_s=round(B / m_off * 1e3), on_pairs_per_s=round(B / m_on * 1e3),
                          on_over_off=round(m_on / m_off, 4), shifts_same_bits=same,
                          median_response=round(float(quality[..., 0].nanmedian()), 4))), flush=True)
    del video, fm, plain, shifts, quality
