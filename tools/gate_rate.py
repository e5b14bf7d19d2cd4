#!/usr/bin/env python3
"""What the FFT engine's response gate (include/mof.h, mof_fft_set_min_response) costs: pairs/s at bench.py's geometries c2, ref, reflr
(the long-range entry of ref's geometry), l200 (pair entries) and c2seq (video entry) in three states -- unarmed, unarmed with the quality
output, armed without a caller quality buffer (the engine's own) -- and the latency of the stateful single-frame call, unarmed and armed.
Quoted in README.md and profiles/fft_min_response.txt; never bench.py's `value`.
usage (GPU box): python tools/gate_rate.py [reps] [workload ...]        -> one JSON line per workload, then one for the stateful call
                 python tools/gate_rate.py step <workload> <min_response>  one warm-up and one call, for a kernel trace

The three states run on the same frames, alternating call by call, each call timed with device events; three rounds of `reps` calls, the
rate is pairs / the median of the rounds' medians. `armed_bits_follow_the_gate` confirms that the armed shifts are the unarmed ones with
NaN where !(response >= min_response)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mrs_optic_flow_amd import FftMethod, synth

WORKLOADS = {
    "c2": dict(h=480, w=752, n=64, grid=(8, 8), origin=(1, 1), stride=(98, 59), batch=1024, entry="pairs"),
    "ref": dict(h=480, w=480, n=120, grid=(4, 4), origin=(0, 0), stride=(120, 120), batch=1024, entry="pairs"),
    "reflr": dict(h=480, w=480, n=120, grid=(4, 4), origin=(0, 0), stride=(120, 120), batch=1024, entry="long_range"),
    "l200": dict(h=480, w=480, n=200, grid=(2, 2), origin=(0, 0), stride=(200, 200), batch=512, entry="pairs"),
    "c2seq": dict(h=480, w=752, n=64, grid=(8, 8), origin=(1, 1), stride=(98, 59), batch=1024, entry="video"),
}
MIN_RESPONSE = 0.3  # (between the classes of INTEGRATION.md's table under cv::phaseCorrelate's model)
dev = torch.device("cuda:0")


def entry_of(fm, w, video):
    if w["entry"] == "video":
        return lambda rq=False: fm.process_sequence_device(video, return_quality=rq)
    if w["entry"] == "long_range":
        return lambda rq=False: fm.process_long_range_batch_device(video[1:], video[:-1], return_quality=rq)
    return lambda rq=False: fm.process_batch_device(video[1:], video[:-1], return_quality=rq)


def timed_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def engine(w):
    return FftMethod(sample_point_size=w["n"], frame_shape=(w["h"], w["w"]), grid=w["grid"], origin=w["origin"], stride=w["stride"])


def main(args):
    if args and args[0] == "step":
        w = WORKLOADS[args[1]]
        fm = engine(w)
        fm.set_min_response(float(args[2]))
        video, _ = synth.video_torch(w["batch"] + 1, w["h"], w["w"], dev, k=1)
        call = entry_of(fm, w, video)
        call()
        call()
        torch.cuda.synchronize()
        return
    reps = max(10, int(args[0])) if args and args[0].isdigit() else 20
    names = [a for a in args if not a.isdigit()] or list(WORKLOADS)
    for name in names:
        w = WORKLOADS[name]
        B = w["batch"]
        video, _ = synth.video_torch(B + 1, w["h"], w["w"], dev, k=1)
        plain, armed = engine(w), engine(w)
        armed.set_min_response(MIN_RESPONSE)
        off, gate = entry_of(plain, w, video), entry_of(armed, w, video)
        states = {"unarmed": off, "unarmed_quality": lambda: off(True), "armed": gate}
        for _ in range(3):
            for call in states.values():
                call()
        rounds = {k: [] for k in states}
        for _ in range(3):
            t = {k: [] for k in states}
            for _ in range(reps):  # alternating
                for k, call in states.items():
                    t[k].append(timed_ms(call)[0])
            for k in states:
                rounds[k].append(statistics.median(t[k]))
        s0, q0 = off(True)
        s1 = gate()
        torch.cuda.synchronize()
        want = torch.where((q0[..., :1] >= MIN_RESPONSE).expand_as(s0), s0, torch.full_like(s0, float("nan")))
        ms = {k: statistics.median(v) for k, v in rounds.items()}
        print(json.dumps(dict(workload=name, kernel_variant=plain.kernel_variant, pairs=B, patches=int(s0.shape[1]), reps=reps, rounds=3,
                              min_response=MIN_RESPONSE, gated_patches=int(torch.isnan(s1[..., 0]).sum() - torch.isnan(s0[..., 0]).sum()),
                              ms={k: round(v, 4) for k, v in ms.items()}, round_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                              pairs_per_s={k: round(B / v * 1e3) for k, v in ms.items()},
                              armed_over_unarmed=round(ms["armed"] / ms["unarmed"], 4),
                              armed_bits_follow_the_gate=bool(torch.equal(s1.view(torch.int64), want.view(torch.int64))))), flush=True)
        del video, plain, armed, s0, q0, s1, want
    # the stateful single-frame call (upload, kernels, read-back, one synchronisation), ref's geometry: wall time per call
    w = WORKLOADS["ref"]
    frames = synth.video_torch(9, w["h"], w["w"], "cpu", k=1)[0].numpy()
    plain, armed = engine(w), engine(w)
    armed.set_min_response(MIN_RESPONSE)
    calls = max(200, 10 * reps)
    rounds = {"unarmed": [], "armed": []}
    for r in range(4):  # (round 0 warms up)
        t = {"unarmed": [], "armed": []}
        for i in range(calls):
            for k, fm in (("unarmed", plain), ("armed", armed)):
                t0 = time.perf_counter()
                fm.processImage(frames[i % 9])
                t[k].append((time.perf_counter() - t0) * 1e6)
        if r:
            for k in t:
                rounds[k].append(statistics.median(t[k]))
    us = {k: statistics.median(v) for k, v in rounds.items()}
    print(json.dumps(dict(workload="stateful processImage, ref geometry", calls_per_round=calls, rounds=3, min_response=MIN_RESPONSE,
                          us_per_call={k: round(v, 2) for k, v in us.items()}, round_us={k: [round(x, 2) for x in v] for k, v in rounds.items()},
                          armed_minus_unarmed_us=round(us["armed"] - us["unarmed"], 2))), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
