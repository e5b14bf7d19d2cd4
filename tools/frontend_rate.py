#!/usr/bin/env python3
"""Rates of the camera front end (include/mof.h, mof_frontend_batch_device; csrc/fe_kernel.hip) and of what it feeds -- quoted in
README.md, DESIGN.md section 4 and INTEGRATION.md; never bench.py's `value`.
usage (GPU box): python tools/frontend_rate.py [frames] [reps]    -> one JSON line per workload

  fe_ref / fe_s2 / fe_s4   the kernel alone on `frames` camera frames: median of `reps` (>= 20) warmed launches timed with device
                           events; required bytes = the tapped source rows (CH per output pixel at s = 1, 2 s CH at even s, s CH at
                           odd s > 1) + the output byte; fraction of the 6.29 TB/s measured copy rate
  c5cam                    a (frames + 1)-frame BGR8 752 x 480 video through the front end once (full-frame gray), then c5seq's two
                           entries on the result (FftMethod video at c2's layout, the estimator on the 480^2 centre view), against c5seq
                           on the same gray frames, alternating; ratio = c5seq step time / c5cam step time
  refcam                   the front end (the node's 480^2 crop) + FftMethod's gray video entry at the reference geometry against the
                           fused process_sequence_device_bgr on the crop view"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mrs_optic_flow_amd import CameraFrontEnd, FftMethod, ScaleRotationEstimator, synth

COPY_RATE = 6.29e12  # bytes/s, the measured device-to-device copy rate of one MI355X
N = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
REPS = max(20, int(sys.argv[2]) if len(sys.argv) > 2 else 30)
dev = torch.device("cuda:0")


def times_ms(call, reps=REPS, warm=3):
    for _ in range(warm):
        call()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def kernel_workload(name, h, w, ch, s, crop):
    shape = (N, h, w) if ch == 1 else (N, h, w, 3)
    frames = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
    fe = CameraFrontEnd((h, w), ch, s, crop)
    out = torch.empty((N,) + fe.out_shape, dtype=torch.uint8, device=dev)
    ms = statistics.median(times_ms(lambda: fe.process_batch_device(frames, out=out)))
    per_px = ch if s == 1 else (2 * s * ch if s % 2 == 0 else s * ch)
    nbytes = (per_px + 1) * crop[2] * crop[3] * N
    print(json.dumps(dict(workload=name, frames=N, camera=[w, h], channels=ch, scale=s, crop=list(crop), kernel_ms=round(ms, 4),
                          required_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3), copy_rate_fraction=round(nbytes / ms * 1e3 / COPY_RATE, 3))),
          flush=True)
    del frames, out


def bgr_video(n, h, w):
    v, _ = synth.video_torch(n, h, w, dev, k=1)
    v = v.to(torch.int32)
    return torch.stack([v, 255 - v, (v * 3) % 256], dim=-1).to(torch.uint8).contiguous()


def c5cam_and_refcam():
    video = bgr_video(N + 1, 480, 752)
    full = CameraFrontEnd((480, 752), 3, 1)
    gray = full.process_batch_device(video).clone()  # c5seq's input: the same frames already gray
    fm = FftMethod(sample_point_size=64, frame_shape=(480, 752), grid=(8, 8), origin=(1, 1), stride=(98, 59))
    sr_a = ScaleRotationEstimator(480, 49.9, batch_chunk=1024)
    sr_b = ScaleRotationEstimator(480, 49.9, batch_chunk=1024)
    out_a = torch.empty((N, fm.n_patches, 2), dtype=torch.float64, device=dev)
    out_b = torch.empty_like(out_a)
    g_cam = torch.empty_like(gray)
    sr_a.process_sequence_device(gray[:2, :, 136:616])  # arm both estimators: every timed frame goes through INTER_LANCZOS4
    sr_b.process_sequence_device(gray[:2, :, 136:616])

    def c5seq():
        fm.process_sequence_device(gray, out=out_a)
        sr_a.process_sequence_device(gray[1:, :, 136:616], resolve_gate=False)

    def c5cam():
        full.process_batch_device(video, out=g_cam)
        fm.process_sequence_device(g_cam, out=out_b)
        sr_b.process_sequence_device(g_cam[1:, :, 136:616], resolve_gate=False)

    t_seq, t_cam = [], []
    for _ in range(3):
        c5seq()
        c5cam()
    for _ in range(REPS):  # alternating
        t_seq += times_ms(c5seq, reps=1, warm=0)
        t_cam += times_ms(c5cam, reps=1, warm=0)
    torch.cuda.synchronize()
    assert torch.equal(out_a.nan_to_num(7.0), out_b.nan_to_num(7.0))
    ms_seq, ms_cam = statistics.median(t_seq), statistics.median(t_cam)
    print(json.dumps(dict(workload="c5cam", frames=N + 1, c5seq_ms=round(ms_seq, 4), c5cam_ms=round(ms_cam, 4),
                          ratio_vs_c5seq=round(ms_seq / ms_cam, 3), target=0.85)), flush=True)

    ref = CameraFrontEnd.reference((480, 752), 3, 1, 480, 376.6)
    x, y, cw, ch = ref.crop
    fr = FftMethod(480, 120)
    g_ref = torch.empty((N + 1, ch, cw), dtype=torch.uint8, device=dev)
    out_c = torch.empty((N, fr.n_patches, 2), dtype=torch.float64, device=dev)
    view = video[:, y:y + ch, x:x + cw]

    def front_end_then_gray():
        ref.process_batch_device(video, out=g_ref)
        fr.process_sequence_device(g_ref, out=out_c)

    def fused():
        return fr.process_sequence_device_bgr(view)

    t_fe, t_fused = [], []
    for _ in range(3):
        front_end_then_gray()
        fused()
    for _ in range(REPS):
        t_fe += times_ms(front_end_then_gray, reps=1, warm=0)
        t_fused += times_ms(fused, reps=1, warm=0)
    ms_fe, ms_fused = statistics.median(t_fe), statistics.median(t_fused)
    print(json.dumps(dict(workload="refcam", frames=N + 1, front_end_plus_gray_ms=round(ms_fe, 4), fused_bgr_ms=round(ms_fused, 4),
                          fused_speedup=round(ms_fe / ms_fused, 3))), flush=True)


kernel_workload("fe_ref", 480, 752, 3, 1, (136, 0, 480, 480))
kernel_workload("fe_s2", 960, 1504, 3, 2, (136, 0, 480, 480))
kernel_workload("fe_s4", 1080, 1920, 1, 4, (120, 15, 240, 240))
c5cam_and_refcam()
