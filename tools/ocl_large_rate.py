#!/usr/bin/env python3
"""Rate of the OpenCL peak model (MOF_PEAK_OCL) on patches too large for one CU -- quoted in DESIGN.md section 4; never bench.py's `value`.
usage (GPU box): python tools/ocl_large_rate.py [pairs] [reps] [sizes,...]    -> one JSON line per patch size

For each size n (default 160, 200, 240, 480, 720) the batch entry (mof_fft_process_batch_device) runs `pairs` (1024) pairs of n x n frames,
one patch each, in three forms, alternated repeat by repeat within one call:
  a  the OpenCL model: the planned large-patch pipeline (csrc/pc_large_kernel.hip, L5 - L8)
  b  the cv::phaseCorrelate model on the same planned pipeline: a child process with MOF_FFT_HALF=0 MOF_FFT_LARGE_TUNED=0 (the
     knobs are read once per process), timed on request between the parent's forms
  c  the cv::phaseCorrelate model on its default route (the half-tile kernel up to 192, the estimator's tuned transforms from 200)
Each repeat times ~20 ms of back-to-back batches (the same count for the three forms) with device events after warm-up; pairs/s from
the median, spread = (max - min) / median over the repeats.
a_over_b is the OpenCL model's cost on the same pipeline, c_over_a what the out-of-scope tuned forms would buy it."""
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mrs_optic_flow_amd import FftMethod, synth

dev = torch.device("cuda:0")


def frames(n, pairs):
    """`pairs` pairs of n x n frames on the device: eight distinct pairs of planted shifts, repeated"""
    cur, prev, _, _ = synth.batch_np(8, n, n, 12, k0=n, classes=False)
    reps = (pairs + 7) // 8
    tc = torch.from_numpy(cur).to(dev).repeat(reps, 1, 1)[:pairs].contiguous()
    tp = torch.from_numpy(prev).to(dev).repeat(reps, 1, 1)[:pairs].contiguous()
    return tc, tp


class Form:
    def __init__(self, n, pairs, peak_model):
        self.fm = FftMethod(n, n, 80.0, peak_model=peak_model)
        self.cur, self.prev = frames(n, pairs)
        self.out = torch.empty((pairs, 1, 2), dtype=torch.float64, device=dev)
        for _ in range(3):  # (the first batch sizes the scratch)
            self.run()
        torch.cuda.synchronize()

    def run(self):
        self.fm.process_batch_device(self.cur, self.prev, out=self.out)

    def time_ms(self, calls=1):
        """milliseconds per batch over `calls` batches back to back"""
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            self.run()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / calls


def worker(n, pairs):
    """form b: answers every line on stdin with the time of one batch, until EOF"""
    f = Form(n, pairs, 0)
    print(f.fm.kernel_variant, flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if len(cmd) != 2 or cmd[0] != "t":
            break
        print(f"{f.time_ms(int(cmd[1])):.6f}", flush=True)


def summary(ms, pairs):
    med = statistics.median(ms)
    return pairs / (med / 1e3), (max(ms) - min(ms)) / med


def main():
    pairs = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
    sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [160, 200, 240, 480, 720]
    for n in sizes:
        env = dict(os.environ, MOF_FFT_HALF="0", MOF_FFT_LARGE_TUNED="0")
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", str(n), str(pairs)], env=env,
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        try:
            variant_b = child.stdout.readline().strip()
            fa, fc = Form(n, pairs, 1), Form(n, pairs, 0)
            calls = max(1, min(64, int(round(20.0 / fa.time_ms()))))  # batches per repeat: ~20 ms of form a
            ms = {"a": [], "b": [], "c": []}
            for _ in range(reps):
                ms["a"].append(fa.time_ms(calls))
                child.stdin.write(f"t {calls}\n")
                child.stdin.flush()
                ms["b"].append(float(child.stdout.readline()))
                ms["c"].append(fc.time_ms(calls))
            child.stdin.close()
            if child.wait(timeout=120) != 0:
                raise RuntimeError(f"form b's child process failed at n = {n}")
        finally:
            if child.poll() is None:
                child.kill()
        rate = {k: summary(v, pairs) for k, v in ms.items()}
        print(json.dumps({
            "n": n, "pairs": pairs, "reps": reps, "batches_per_rep": calls,
            "variant": {"a": fa.fm.kernel_variant, "b": variant_b, "c": fc.fm.kernel_variant},
            "pairs_per_s": {k: round(v[0], 1) for k, v in rate.items()},
            "spread": {k: round(v[1], 4) for k, v in rate.items()},
            "a_over_b": round(rate["a"][0] / rate["b"][0], 4),
            "c_over_a": round(rate["c"][0] / rate["a"][0], 4),
        }), flush=True)
        del fa, fc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(int(sys.argv[2]), int(sys.argv[3]))
    else:
        main()
