#!/usr/bin/env python3
"""What the FFT engine's predicted-shift window offsets (include/mof.h, "Predicted-shift window offsets") cost beside the plain batch
entry: time per batch of frame pairs at four geometries, on one box, the contenders alternating call by call.

  plain         mof_fft_process_batch_device
  plain_parent  the same entry of ANOTHER build of the library (--parent-lib PATH: the parent commit's; its kernels are untouched, so the
                same time is expected), measured by child processes before and after the alternated rounds
  pred_zero     mof_fft_process_batch_device_pred, predictions all 0
  pred_pm3      ... predictions uniform in [-3, 3]
  c2f           mof_fft_process_coarse_to_fine_batch_device (reference tilings with a 4 x 4 grid or more)
  lr_then_plain the long-range entry and the plain entry, called one after the other (what a node that wants both pays today)
  plain_copy    the plain entry plus a device-to-device copy of the previous frames (the bytes the gather moves, moved by the runtime)

usage (GPU box): python tools/pred_rate.py [reps] [--parent-lib PATH] [--out FILE] [geometry ...]
                 python tools/pred_rate.py plain-only [reps] [geometry ...]      (what the child processes run)
Writes FILE (default profiles/fft_pred.txt): one JSON line per geometry, then the reading. Each call is timed with device events; three
rounds of `reps` (>= 5) calls per contender, a contender's time is the median of its rounds' medians, its spread the range of them.
The gather moves 2 x the patch bytes (read + write); its rate is quoted against the 6.29 TB/s device copy rate the front end's row uses.
Nothing here is bench.py's `value`."""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOMETRIES = {
    "ref": dict(fs=480, n=120, batch=1024),   # 4 x 4 patches of 120: the reference's default
    "g448": dict(fs=448, n=64, batch=1024),   # 7 x 7 x 64
    "g512": dict(fs=512, n=128, batch=512),   # 4 x 4 x 128
    "g400": dict(fs=400, n=200, batch=256),   # 2 x 2 x 200: no long-range form
}
COPY_TBPS = 6.29
ROUNDS = 3


def timed_ms(call):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(states, reps):
    """{name: call} -> {name: (median of the rounds' medians, [the rounds' medians])}, alternating call by call"""
    for _ in range(3):
        for call in states.values():
            call()
    rounds = {k: [] for k in states}
    for _ in range(ROUNDS):
        t = {k: [] for k in states}
        for _ in range(reps):
            for k, call in states.items():
                t[k].append(timed_ms(call))
        for k in states:
            rounds[k].append(statistics.median(t[k]))
    return {k: (statistics.median(v), v) for k, v in rounds.items()}


def setup(name):
    import torch

    from mrs_optic_flow_amd import FftMethod, synth

    g = GEOMETRIES[name]
    dev = torch.device("cuda:0")
    video, _ = synth.video_torch(g["batch"] + 1, g["fs"], g["fs"], dev, k=1)
    # (prev in a buffer of its own: on cur = prev + one frame the large-patch pipeline would take its video form for the plain entry only)
    return g, FftMethod(g["fs"], g["n"], 80.0), video[1:], video[:-1].clone()


def plain_only(reps, names):
    # another build of the library may lack the newest entries, which the binding would insist on: bind what it exports
    import ctypes

    import torch  # noqa: F401  (before anything loads a HIP runtime: mrs_optic_flow_amd/_capi.py)

    from mrs_optic_flow_amd import _capi

    exported = ctypes.CDLL(_capi.LIB_PATH)
    for table in (_capi.SYMBOLS, _capi.PRED_ROUTE_SYMBOLS):
        for symbol in [s for s in table if not hasattr(exported, s)]:
            del table[symbol]
    for name in names:
        g, fm, cur, prev = setup(name)
        ms, rounds = measure({"plain": lambda: fm.process_batch_device(cur, prev)}, reps)["plain"]
        print(json.dumps(dict(geometry=name, ms=round(ms, 4), round_ms=[round(x, 4) for x in rounds])), flush=True)


def parent_runs(lib, reps, names):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "plain-only", str(reps)] + names, capture_output=True, text=True,
                       env=dict(os.environ, MOF_LIB_PATH=lib), timeout=900)
    if r.returncode != 0:
        raise RuntimeError("plain-only child failed: " + r.stderr[-800:])
    return {d["geometry"]: d for d in (json.loads(line) for line in r.stdout.strip().splitlines())}


def main(args):
    if args and args[0] == "plain-only":
        reps = max(5, int(args[1]))
        return plain_only(reps, args[2:] or list(GEOMETRIES))
    import torch

    parent_lib, out_path, rest = None, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fft_pred.txt"), []
    it = iter(args)
    for a in it:
        if a == "--parent-lib":
            parent_lib = next(it)
        elif a == "--out":
            out_path = next(it)
        else:
            rest.append(a)
    reps = max(5, int(rest[0])) if rest and rest[0].isdigit() else 10
    names = [a for a in rest if not a.isdigit()] or list(GEOMETRIES)
    before = parent_runs(parent_lib, reps, names) if parent_lib else {}
    lines = []
    for name in names:
        g, fm, cur, prev = setup(name)
        B, patches, n = g["batch"], fm.n_patches, g["n"]
        has_lr = fm.cfg.grid_x >= 4 and g["fs"] % 4 == 0
        zeros = torch.zeros((B, patches, 2), dtype=torch.int32, device=cur.device)
        pm3 = torch.randint(-3, 4, (B, patches, 2), dtype=torch.int32, device=cur.device, generator=torch.Generator(cur.device).manual_seed(7))
        spare = torch.empty_like(prev)
        states = {
            "plain": lambda: fm.process_batch_device(cur, prev),
            "pred_zero": lambda: fm.process_batch_device_pred(cur, prev, zeros),
            "pred_pm3": lambda: fm.process_batch_device_pred(cur, prev, pm3),
            "plain_copy": lambda: (spare.copy_(prev), fm.process_batch_device(cur, prev)),
        }
        if has_lr:
            states["c2f"] = lambda: fm.process_coarse_to_fine_batch_device(cur, prev)
            states["lr_then_plain"] = lambda: (fm.process_long_range_batch_device(cur, prev), fm.process_batch_device(cur, prev))
        res = measure(states, reps)
        same = bool(torch.equal(fm.process_batch_device_pred(cur, prev, zeros).view(torch.int64), fm.process_batch_device(cur, prev).view(torch.int64)))
        ms = {k: v[0] for k, v in res.items()}
        spread = {k: max(v[1]) - min(v[1]) for k, v in res.items()}
        gather_ms, copy_ms = ms["pred_zero"] - ms["plain"], ms["plain_copy"] - ms["plain"]
        moved = 2.0 * B * patches * n * n
        rate = moved / (gather_ms * 1e-3) / 1e12 if gather_ms > 0 else float("nan")
        slack = spread["pred_zero"] + spread["plain"] + spread["plain_copy"]
        d = dict(geometry=name, frame=g["fs"], patch=n, patches=patches, pairs=B, kernel_variant=fm.kernel_variant, reps=reps, rounds=ROUNDS,
                 ms={k: round(v, 4) for k, v in ms.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                 pairs_per_s={k: round(B / v * 1e3) for k, v in ms.items()}, pred_minus_plain_ms=round(gather_ms, 4),
                 copy_ms=round(copy_ms, 4), gather_bytes=int(moved), gather_tb_per_s=round(rate, 3),
                 gather_fraction_of_copy_rate=round(rate / COPY_TBPS, 3), pred_minus_plain_within_copy_time=bool(gather_ms <= copy_ms + slack),
                 zero_prediction_bits_equal_plain=same)
        if parent_lib:
            d["plain_parent_ms_before"] = before[name]["ms"]
        lines.append(d)
        print(json.dumps(d), flush=True)
        del fm, cur, prev, zeros, pm3, spare, states
        torch.cuda.empty_cache()
    if parent_lib:
        after = parent_runs(parent_lib, reps, names)
        for d in lines:
            d["plain_parent_ms_after"] = after[d["geometry"]]["ms"]
    with open(out_path, "w") as f:
        f.write("FFT engine, predicted-shift window offsets: time per batch (tools/pred_rate.py; one box, contenders alternated call by call,\n"
                f"medians of {ROUNDS} rounds of {reps} calls, device events). ms per batch of `pairs` frame pairs.\n\n")
        for d in lines:
            f.write(json.dumps(d) + "\n")
        f.write("\nReading: pred_minus_plain_ms is the gather and finish kernels' time (zero predictions: the same field kernels on the same\n"
                "pixels); copy_ms is what the runtime's device copy of the previous frames adds to the plain entry. gather_tb_per_s counts the\n"
                f"2 x patch bytes the gather reads and writes; the fraction is of the {COPY_TBPS} TB/s copy rate the front end's row is quoted\n"
                "against. pred_minus_plain_within_copy_time: pred - plain <= copy time + the three contenders' spreads.\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main(sys.argv[1:])
