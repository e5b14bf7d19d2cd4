#!/usr/bin/env python3
"""What the block matchers' quality outputs and match gate (include/mof.h, mof_bm_*_q, mof_bm_set_gate) cost: pairs/s of the device batch
entry at bench.py's geometries c1, c3, bmref and c3bgr in three states -- off (no quality pointer, gate off: the kernels the parent
commit launches), quality (return_quality=True, gate off) and armed (gate on, no quality pointer) -- and `off` against the parent commit's
own tree. Quoted in README.md and profiles/bm_quality.txt; never bench.py's `value`.
usage (GPU box): python tools/bm_quality_rate.py [reps] [workload ...]   one JSON line per workload: the three states in one process
                 python tools/bm_quality_rate.py ab [reps] [workload ...]  `off` in the parent's tree (tmp_ab/parent, prepared where hipcc
                                                                           is by tools/ab_commit.sh prepare <commit>) and in this one,
                                                                           one process each, alternating old / new three times
                 python tools/bm_quality_rate.py off <workload> <reps>     one such process: prints the median ms of `off` (MOF_AB_TREE
                                                                           names the tree whose package is imported)

The states run on the same frames and alternate call by call, each call timed with device events; three rounds of `reps` calls, the rate is
pairs / the median of the rounds' medians. The armed thresholds are per-pixel figures between the classes of INTEGRATION.md's table, scaled
by block_size^2; `armed_follows_quality` confirms on the device that the armed shifts are the off shifts with -128 where the quality
output fails the two compares."""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("MOF_AB_TREE") or ROOT)
import torch  # noqa: E402

from mrs_optic_flow_amd import BlockMethod, FastSpacedBMMethod, synth  # noqa: E402

WORKLOADS = {
    "c1": dict(block_method=True, h=272, w=272, block=32, step=0, radius=8, batch=1024),
    "c3": dict(h=480, w=752, block=16, step=8, radius=16, batch=1024),
    "bmref": dict(h=480, w=752, block=120, step=24, radius=21, batch=256),
    "c3bgr": dict(bgr=True, h=480, w=752, block=16, step=8, radius=16, batch=512),
}
MAX_MIN_SAD_PX, MIN_SAD_RANGE_PX = 20, 30  # grey levels per pixel: matched blocks 2 .. 3 / 46 .. 66, unrelated views 37 .. 49 / 6 .. 26
dev = torch.device("cuda:0")


def engine(w):
    if w.get("block_method"):
        return BlockMethod(w["h"], w["block"], w["radius"])
    return FastSpacedBMMethod(w["block"], w["radius"], w["step"], (w["h"], w["w"]))


def frames(w):
    video, _ = synth.video_torch(w["batch"] + 1, w["h"], w["w"], dev, k=1)
    cur, prev = video[1:], video[:-1]
    if w.get("bgr"):  # bench.py's colour frames: three affine maps of the gray texture
        def colour(g):
            g16 = g.to(torch.int16)
            return torch.stack([g, (255 - g16 // 2).to(torch.uint8), (g16 * 3 // 4 + 20).to(torch.uint8)], dim=-1).contiguous()
        return colour(cur), colour(prev)
    return cur, prev


def entry_of(eng, w, cur, prev):
    fn = eng.process_batch_device_bgr if w.get("bgr") else eng.process_batch_device
    return lambda **kw: fn(cur, prev, **kw)


def timed_ms(call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def rounds_of(states, reps):
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
    return rounds


def three_states(name, reps):
    w = WORKLOADS[name]
    B, px = w["batch"], w["block"] ** 2
    cur, prev = frames(w)
    plain, armed = engine(w), engine(w)
    a, r = MAX_MIN_SAD_PX * px, MIN_SAD_RANGE_PX * px
    armed.set_gate(a, r)
    off, gate = entry_of(plain, w, cur, prev), entry_of(armed, w, cur, prev)
    rounds = rounds_of({"off": off, "quality": lambda: off(return_quality=True), "armed": gate}, reps)
    dx0, dy0, _, (q, _) = off(return_quality=True)
    dx1, dy1, _ = gate()
    torch.cuda.synchronize()
    valid = (q[..., 0] <= a) & (q[..., 2] - q[..., 0] >= r)
    inv = torch.full_like(dx0, -128)
    follows = bool(torch.equal(dx1, torch.where(valid, dx0, inv)) and torch.equal(dy1, torch.where(valid, dy0, inv)))
    ms = {k: statistics.median(v) for k, v in rounds.items()}
    print(json.dumps(dict(workload=name, pairs=B, blocks=int(dx0.shape[1] * dx0.shape[2]), reps=reps, rounds=3, gate=[a, r],
                          gated_blocks=int((~valid).sum()), ms={k: round(v, 4) for k, v in ms.items()},
                          round_ms={k: [round(x, 4) for x in v] for k, v in rounds.items()},
                          pairs_per_s={k: round(B / v * 1e3) for k, v in ms.items()},
                          quality_over_off=round(ms["quality"] / ms["off"], 4), armed_over_off=round(ms["armed"] / ms["off"], 4),
                          armed_follows_quality=follows)), flush=True)


def off_only(name, reps):
    w = WORKLOADS[name]
    cur, prev = frames(w)
    rounds = rounds_of({"off": entry_of(engine(w), w, cur, prev)}, reps)["off"]
    print(json.dumps(dict(ms=round(statistics.median(rounds), 4), round_ms=[round(x, 4) for x in rounds])), flush=True)


def ab(names, reps):
    parent = os.path.join(ROOT, "tmp_ab", "parent")
    if not os.path.exists(os.path.join(parent, "mrs_optic_flow_amd", "libmof_hip.so")):
        sys.exit("run 'tools/ab_commit.sh prepare <commit>' where hipcc is first")
    for name in names:
        ms = {"old": [], "new": []}
        for _ in range(3):
            for v, tree in (("old", parent), ("new", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "off", name, str(reps)], capture_output=True, text=True, timeout=240,
                                   cwd=tree, env=dict(os.environ, MOF_AB_TREE=tree))
                if r.returncode != 0:
                    sys.exit(f"{v} run of {name} failed ({r.returncode}): stopping\n{r.stderr[-2000:]}")
                ms[v].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        B = WORKLOADS[name]["batch"]
        med = {v: statistics.median(x) for v, x in ms.items()}
        print(json.dumps(dict(workload=name, state="off", pairs=B, reps=reps, process_ms=ms,
                              pairs_per_s={v: round(B / m * 1e3) for v, m in med.items()},
                              spread={v: round((max(x) - min(x)) / statistics.median(x), 4) for v, x in ms.items()},
                              new_over_old=round(med["new"] / med["old"], 4))), flush=True)


def main(args):
    if args and args[0] == "off":
        return off_only(args[1], int(args[2]))
    mode_ab = bool(args) and args[0] == "ab"
    args = args[1:] if mode_ab else args
    reps = max(10, int(args[0])) if args and args[0].isdigit() else 20
    names = [a for a in args if not a.isdigit()] or list(WORKLOADS)
    if mode_ab:
        return ab(names, reps)
    for name in names:
        three_states(name, reps)


if __name__ == "__main__":
    main(sys.argv[1:])
