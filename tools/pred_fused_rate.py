#!/usr/bin/env python3
"""What the two routes of the FFT engine's window-offset entries (include/mof.h: MOF_PRED_ROUTE_GATHER, MOF_PRED_ROUTE_FUSED) cost beside
the plain batch entry: time per batch of frame pairs, on one box, the contenders alternating call by call -- the method of
tools/pred_rate.py (profiles/fft_pred.txt), whose four layouts come first; then c2 and c4 of bench.py themselves, overlapping layouts
that only the fused route serves.

  plain               mof_fft_process_batch_device
  gather_zero / _pm3  mof_fft_process_batch_device_pred on the gather route, predictions all 0 / uniform in [-3, 3]
  fused_zero / _pm3   the same on the fused route (an engine of its own; none where the layout's kernels have no fused form)
  c2f_gather / _fused mof_fft_process_coarse_to_fine_batch_device on either route (reference tilings with a 4 x 4 grid or more)

usage (GPU box): python tools/pred_fused_rate.py [reps] [--out FILE] [layout ...]
Writes FILE (default profiles/fft_pred_fused.txt): one JSON line per layout, then the reading. Each call is timed with device events;
three rounds of `reps` (>= 5) calls per contender, a contender's time is the median of its rounds' medians, its spread the range of them.
The hypothesis on record: at ref and g512, fused - plain lies below gather - plain by more than the two routes' combined spread.
Nothing here is bench.py's `value`."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pred_rate import ROUNDS, measure  # noqa: E402

LAYOUTS = {
    "ref": dict(h=480, w=480, n=120, batch=1024),   # 4 x 4 patches of 120: the reference's default
    "g448": dict(h=448, w=448, n=64, batch=1024),   # 7 x 7 x 64
    "g512": dict(h=512, w=512, n=128, batch=512),   # 4 x 4 x 128
    "g400": dict(h=400, w=400, n=200, batch=256),   # 2 x 2 x 200: the large-patch pipeline, no fused form
    # bench.py's c2 and c4: patches overlap, the gather route returns MOF_ERR_UNSUPPORTED
    "c2": dict(h=480, w=752, n=64, grid=(8, 8), origin=(1, 1), stride=(98, 59), batch=1024),
    "c4": dict(h=1080, w=1920, n=128, grid=(16, 16), origin=(0, 0), stride=(119, 63), batch=256),
}


def engine(g):
    from mrs_optic_flow_amd import FftMethod

    if "grid" in g:
        return FftMethod(sample_point_size=g["n"], max_px_speed=80.0, frame_shape=(g["h"], g["w"]), grid=g["grid"], origin=g["origin"], stride=g["stride"])
    return FftMethod(g["h"], g["n"], 80.0)


def main(args):
    import torch

    from mrs_optic_flow_amd import synth

    out_path, rest = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fft_pred_fused.txt"), []
    it = iter(args)
    for a in it:
        if a == "--out":
            out_path = next(it)
        else:
            rest.append(a)
    reps = max(5, int(rest[0])) if rest and rest[0].isdigit() else 10
    names = [a for a in rest if not a.isdigit()] or list(LAYOUTS)
    dev = torch.device("cuda:0")
    lines = []
    for name in names:
        g = LAYOUTS[name]
        video, _ = synth.video_torch(g["batch"] + 1, g["h"], g["w"], dev, k=1)
        cur, prev = video[1:], video[:-1].clone()  # (prev in a buffer of its own, as tools/pred_rate.py)
        fm, ff = engine(g), engine(g)
        overlap = fm.cfg.stride_x < g["n"] or fm.cfg.stride_y < g["n"]
        has_fused = fm.pred_route_supported("fused")
        if has_fused:
            ff.set_pred_route("fused")
        B, patches = g["batch"], fm.n_patches
        has_lr = not overlap and fm.cfg.grid_x >= 4 and g["h"] % 4 == 0 and "grid" not in g
        zeros = torch.zeros((B, patches, 2), dtype=torch.int32, device=dev)
        pm3 = torch.randint(-3, 4, (B, patches, 2), dtype=torch.int32, device=dev, generator=torch.Generator(dev).manual_seed(7))
        states = {"plain": lambda: fm.process_batch_device(cur, prev)}
        if not overlap:
            states["gather_zero"] = lambda: fm.process_batch_device_pred(cur, prev, zeros)
            states["gather_pm3"] = lambda: fm.process_batch_device_pred(cur, prev, pm3)
        if has_fused:
            states["fused_zero"] = lambda: ff.process_batch_device_pred(cur, prev, zeros)
            states["fused_pm3"] = lambda: ff.process_batch_device_pred(cur, prev, pm3)
        if has_lr:
            states["c2f_gather"] = lambda: fm.process_coarse_to_fine_batch_device(cur, prev)
            if has_fused:
                states["c2f_fused"] = lambda: ff.process_coarse_to_fine_batch_device(cur, prev)
        res = measure(states, reps)
        ms = {k: v[0] for k, v in res.items()}
        spread = {k: max(v[1]) - min(v[1]) for k, v in res.items()}
        d = dict(layout=name, frame=[g["w"], g["h"]], patch=g["n"], patches=patches, pairs=B, kernel_variant=fm.kernel_variant, overlapping=bool(overlap),
                 fused_supported=bool(has_fused), reps=reps, rounds=ROUNDS, ms={k: round(v, 4) for k, v in ms.items()},
                 spread_ms={k: round(v, 4) for k, v in spread.items()}, pairs_per_s={k: round(B / v * 1e3) for k, v in ms.items()})
        if has_fused:
            plain_bits = fm.process_batch_device(cur, prev).view(torch.int64)
            d["fused_zero_bits_equal_plain"] = bool(torch.equal(ff.process_batch_device_pred(cur, prev, zeros).view(torch.int64), plain_bits))
            d["fused_minus_plain_ms"] = {k: round(ms["fused_" + k] - ms["plain"], 4) for k in ("zero", "pm3")}
        if not overlap:
            d["gather_minus_plain_ms"] = {k: round(ms["gather_" + k] - ms["plain"], 4) for k in ("zero", "pm3")}
        if has_fused and not overlap:
            d["fused_pm3_bits_equal_gather"] = bool(torch.equal(ff.process_batch_device_pred(cur, prev, pm3).view(torch.int64),
                                                                fm.process_batch_device_pred(cur, prev, pm3).view(torch.int64)))
            for k in ("zero", "pm3"):
                gap = (ms["gather_" + k] - ms["plain"]) - (ms["fused_" + k] - ms["plain"])
                both = spread["gather_" + k] + spread["fused_" + k]
                d["gather_minus_fused_ms_" + k] = round(gap, 4)
                d["combined_spread_ms_" + k] = round(both, 4)
                d["fused_below_gather_by_more_than_spread_" + k] = bool(gap > both)
        lines.append(d)
        print(json.dumps(d), flush=True)
        del fm, ff, cur, prev, video, zeros, pm3, states
        torch.cuda.empty_cache()
    with open(out_path, "w") as f:
        f.write("FFT engine, window offsets on the gather and the fused route: time per batch (tools/pred_fused_rate.py; one box, contenders\n"
                f"alternated call by call, medians of {ROUNDS} rounds of {reps} calls, device events). ms per batch of `pairs` frame pairs.\n\n")
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write("\nReading: *_minus_plain_ms is what a route adds to the plain entry of the same run (gather: the gather and finish kernels;\n"
                "fused: the clamp and finish kernels and whatever the displaced loads cost inside the field kernel). gather_minus_fused_ms is\n"
                "the difference of the two, combined_spread_ms the sum of the two contenders' round-to-round ranges; the hypothesis holds for a\n"
                "layout where fused_below_gather_by_more_than_spread_* is true. Overlapping layouts (c2, c4) have no gather contender: the\n"
                "gather route refuses them. g400 runs the large-patch pipeline, which has no fused form.\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1:])
