#!/usr/bin/env python3
"""The peak tails' outputs on a fixed corpus, for a bit-for-bit comparison of two builds of the library (tools/ab_commit.sh bits).
usage: python tools/tail_bits.py run OUT.npz       (GPU box; the library is the one MOF_LIB_PATH names, else the tree's own)
       python tools/tail_bits.py compare A.npz B.npz   (CPU: array_equal with equal NaNs on every array; exit status 1 on a difference)

The corpus goes through every tail of csrc/pc_common.hpp (peak_window / peak_finish / spectrum_window / sr_finish) and every pixel
front end that shares its byte extraction: the batches of tests/quality_cases.py through the quality entries (the sequence entry
for the video batches, the OpenCL model for the ocl-* ones), the 36 circular-shift pairs under the OpenCL model with no mask, BGR8
batches, the long-range mode, constant and all-zero patches against texture on padded sizes, the scale / rotation estimator on
tests/sr_scenes.py views with black frames, one BGR8 block-matching batch; and through every front-end form of every FFT launcher on
the default route (tests/launch_form_cases.py: gray, BGR8 and long-range under both peak models, pairs and videos)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def _bgr(gray, seed):
    """an interleaved BGR8 batch around a gray one: each channel the gray value plus its own tint in [0, 40)"""
    tint = np.random.default_rng(seed).integers(0, 40, gray.shape + (3,))
    return np.clip(gray[..., None].astype(np.int64) + tint, 0, 255).astype(np.uint8)


def run(path):
    import torch

    import quality_cases as Q
    import sr_scenes
    from mrs_optic_flow_amd import FastSpacedBMMethod, FftMethod, ScaleRotationEstimator
    from mrs_optic_flow_amd.engine import PEAK_OCL

    dev = torch.device("cuda:0")
    out = {}

    def put(name, *tensors):
        for i, t in enumerate(tensors):
            out[f"{name}/{i}"] = t.cpu().numpy()

    def gpu(a):
        return torch.from_numpy(np.array(a)).to(dev)  # (a copy: the shared batches are read-only)

    def one_patch(n, **kw):
        return FftMethod(sample_point_size=n, max_px_speed=Q.SPEED, frame_shape=(n, n), grid=(1, 1), **kw)

    for name, build in Q.BATCHES.items():
        b = build()
        if name == "long-range":
            put(name, *FftMethod(128, 32, Q.SPEED).process_long_range_batch_device(gpu(b.cur), gpu(b.prev), return_quality=True))
            continue
        h, w = b.cur.shape[1:3]
        fm = FftMethod(sample_point_size=b.n, max_px_speed=Q.SPEED, frame_shape=(h, w), grid=b.grid, peak_model=PEAK_OCL if b.ocl else 0)
        if name.startswith("video-"):
            put(name, *fm.process_sequence_device(gpu(b.frames), return_quality=True))
        else:
            put(name, *fm.process_batch_device(gpu(b.cur), gpu(b.prev), return_quality=True))
    import launch_form_cases as L
    for name, case in L.CASES.items():  # every front-end form of every FFT launcher on the default route (3 frames or 2 pairs each)
        put(f"form-{name}", *L.run(case, L.engine(case), dev, return_quality=True))
    for n in (64, 60, 144):  # the 7 x 7 window clamped at the surface's edges (tests/test_gpu_peak_tail.py)
        cur, prev = Q.circular_pairs(n)
        put(f"ocl-circular-{n}", *one_patch(n, peak_model=PEAK_OCL, search_radius=n).process_batch_device(gpu(cur), gpu(prev), return_quality=True))
    for n in (64, 54, 120, 196):
        cur, prev = Q.crop_pairs(n, n, 6, seed=700 + n)
        put(f"bgr-{n}", *one_patch(n).process_batch_device_bgr(gpu(_bgr(cur, n)), gpu(_bgr(prev, n + 1)), return_quality=True))
    for n in (60, 200):
        cur, prev = Q.crop_pairs(4 * n, 4 * n, 3, seed=800 + n, step=4)
        put(f"long-range-{n}", *FftMethod(4 * n, n, Q.SPEED).process_long_range_batch_device(gpu(cur), gpu(prev), return_quality=True))
    for n in (62, 142, 196):
        tex = np.random.default_rng(11).integers(0, 256, (n, n), dtype=np.uint8)
        const, zero = np.full((n, n), 81, np.uint8), np.zeros((n, n), np.uint8)
        cur, prev = np.stack([const, tex, zero, tex]), np.stack([tex, const, tex, zero])
        put(f"constant-{n}", *one_patch(n).process_batch_device(gpu(cur), gpu(prev), return_quality=True))
    for res in (240, 208, 64):
        base = sr_scenes.canvas(7, res)
        views = [sr_scenes.view(base, res, sc, ro) for sc, ro in [(1.0, 0.0), (1.04, 3.0), (0.95, -6.0), (1.0, 9.0), (1.1, 1.0)]]
        black = np.zeros((res, res), np.uint8)
        cur, prev = np.stack(views[1:] + [black, views[0], black]), np.stack(views[:-1] + [views[0], black, black])
        put(f"estimator-{res}", ScaleRotationEstimator(res, 40.0).process_batch_device(gpu(cur), gpu(prev)))
    cur, prev = Q.crop_pairs(160, 224, 3, seed=900)
    put("bm-bgr", *FastSpacedBMMethod(16, 16, 8, (160, 224)).process_batch_device_bgr(gpu(_bgr(cur, 1)), gpu(_bgr(prev, 2))))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path} ({os.environ.get('MOF_LIB_PATH') or 'the tree library'})")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    assert sorted(a.files) == sorted(b.files), (sorted(set(a.files) ^ set(b.files)))
    bad = 0
    for k in sorted(a.files):
        x, y = a[k], b[k]
        same = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=x.dtype.kind == "f")
        if same and x.dtype.kind == "f":  # (array_equal takes +0 for -0)
            same = np.array_equal(np.signbit(x), np.signbit(y))
        if not same:
            bad += 1
            where = np.argwhere(~((x == y) | (np.isnan(x) & np.isnan(y)))).tolist() if x.shape == y.shape else "shape"
            print(f"DIFFERENT {k}: {where}")
    nan = sum(int(np.isnan(a[k]).sum()) for k in a.files if a[k].dtype.kind == "f")
    print(f"{len(a.files)} arrays, {sum(a[k].size for k in a.files)} values ({nan} NaN): {'all equal' if bad == 0 else f'{bad} arrays differ'}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run":
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
