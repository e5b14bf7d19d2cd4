"""GPU tests of the camera front end (include/mof.h, mof_frontend_*; csrc/fe_kernel.hip): byte-exact against the numpy restatement
(tests/frontend_ref.py, anchored to the oracle by tests/test_frontend_host.py), bit-identical composition with the fused BGR entries
at s = 1, the consumers it opens to camera frames, graph capture, and refusals that launch nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import frontend_ref
from mrs_optic_flow_amd import (BlockMethod, CameraFrontEnd, FastSpacedBMMethod, FftMethod, MofError, ScaleRotationEstimator, _capi,
                                release_captured, synth)

pytestmark = pytest.mark.gpu


def _same(a, b) -> bool:
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _strided_frames(rng, n, h, w, ch, pad=13, gap=7, device="cuda:0"):
    """n random camera frames with rows pad bytes longer than the image and gap bytes between frames -> (tensor view, numpy)."""
    pitch = ch * w + pad
    stride = h * pitch + gap
    flat = torch.from_numpy(rng.integers(0, 256, n * stride + 64, dtype=np.uint8)).to(device)
    if ch == 1:
        view = flat[5:].as_strided((n, h, w), (stride, pitch, 1))
    else:
        view = flat[5:].as_strided((n, h, w, 3), (stride, pitch, 3, 1))
    return view, view.cpu().numpy()


def _bgr_video(n, h, w, k=0):
    """a BGR8 video whose gray image moves like synth.video_torch's frames (each channel a pointwise function of one frame)."""
    v, _ = synth.video_torch(n, h, w, "cpu", k=k)
    v = v.to(torch.int32)
    return torch.stack([v, 255 - v, (v * 3) % 256], dim=-1).to(torch.uint8).contiguous()


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 6, 7, 8])
def test_bytes_match_the_restatement(gpu, channels, s):
    rng = np.random.default_rng(100 * s + channels)
    n, ws, hs = 3, 53, 29
    frames, fnp = _strided_frames(rng, n, hs * s, ws * s, channels)
    for crop in ((3, 5, 45, 21), (0, 0, ws, hs), (1, 1, 37, 9), (50, 28, 3, 1)):
        fe = CameraFrontEnd((hs * s, ws * s), channels, s, crop)
        want = frontend_ref.frontend(fnp, s, crop)
        got = fe.process_batch_device(frames).cpu().numpy()
        assert np.array_equal(got, want), (s, channels, crop)
        # an output pitch wider than the crop: the padding is not written
        buf = torch.full((n, crop[3], crop[2] + 9), 0xA5, dtype=torch.uint8, device=gpu)
        fe.process_batch_device(frames, out=buf[:, :, :crop[2]])
        b = buf.cpu().numpy()
        assert np.array_equal(b[:, :, :crop[2]], want) and (b[:, :, crop[2]:] == 0xA5).all()


def test_batch_beyond_one_launch(gpu):
    """70,000 frames: more frames than one launch takes (65535)."""
    rng = np.random.default_rng(7)
    n = 70000
    frames = torch.from_numpy(rng.integers(0, 256, (n, 6, 8, 3), dtype=np.uint8)).to(gpu)
    fe = CameraFrontEnd((6, 8), 3, 2, (1, 0, 3, 2))
    got = fe.process_batch_device(frames).cpu().numpy()
    assert np.array_equal(got, frontend_ref.frontend(frames.cpu().numpy(), 2, (1, 0, 3, 2)))


def test_fft_sequence_identical_to_the_fused_bgr_entry(gpu):
    video = _bgr_video(6, 480, 752, k=1).to(gpu)
    # the reference geometry: 752 x 480 camera -> 480^2 crop, 4 x 4 patches of 120^2
    fe = CameraFrontEnd.reference((480, 752), 3, 1, 480, 376.6)
    x, y, cw, ch = fe.crop
    fm = FftMethod(480, 120)
    assert _same(fm.process_sequence_device(fe.process_batch_device(video)),
                 fm.process_sequence_device_bgr(video[:, y:y + ch, x:x + cw]))
    # c2's layout on the whole frame
    full = CameraFrontEnd((480, 752), 3, 1)
    c2 = FftMethod(sample_point_size=64, frame_shape=(480, 752), grid=(8, 8), origin=(1, 1), stride=(98, 59))
    gray = full.process_batch_device(video)
    assert _same(c2.process_sequence_device(gray), c2.process_sequence_device_bgr(video))
    assert _same(c2.process_batch_device(gray[1:], gray[:-1]), c2.process_batch_device_bgr(video[1:], video[:-1]))


def test_block_matching_identical_to_the_fused_bgr_entry(gpu):
    video = _bgr_video(5, 480, 752, k=2).to(gpu)
    gray = CameraFrontEnd((480, 752), 3, 1).process_batch_device(video)
    bm = FastSpacedBMMethod(16, 16, 8, (480, 752))
    for a, b in zip(bm.process_batch_device(gray[1:], gray[:-1]), bm.process_batch_device_bgr(video[1:], video[:-1])):
        assert torch.equal(a, b)


def _restated(video, s, crop):
    return torch.from_numpy(frontend_ref.frontend(video.cpu().numpy(), s, crop)).to(video.device)


def test_estimator_on_camera_frames(gpu):
    # s = 1: the node's 480^2 crop of a 752 x 480 camera
    video = _bgr_video(6, 480, 752, k=3).to(gpu)
    fe = CameraFrontEnd.reference((480, 752), 3, 1, 480, 376.6)
    got = ScaleRotationEstimator(480, 49.9).process_sequence_device(fe.process_batch_device(video))
    want = ScaleRotationEstimator(480, 49.9).process_sequence_device(_restated(video, 1, fe.crop))
    assert _same(got, want)
    # s = 2: a 1504 x 960 camera, an explicit crop centred on cx / s (the node's own rectangle leaves the image, see the header)
    big = _bgr_video(5, 960, 1504, k=4).to(gpu)
    fe2 = CameraFrontEnd((960, 1504), 3, 2, (256, 120, 240, 240))
    got = ScaleRotationEstimator(240, 40.0).process_sequence_device(fe2.process_batch_device(big))
    want = ScaleRotationEstimator(240, 40.0).process_sequence_device(_restated(big, 2, fe2.crop))
    assert _same(got, want)


def test_long_range_mode_on_camera_frames(gpu):
    video = _bgr_video(5, 480, 752, k=5).to(gpu)
    fe = CameraFrontEnd.reference((480, 752), 3, 1, 480, 376.6)
    gray, ref = fe.process_batch_device(video), _restated(video, 1, fe.crop)
    fm = FftMethod(480, 120)
    assert _same(fm.process_long_range_batch_device(gray[1:], gray[:-1]), fm.process_long_range_batch_device(ref[1:], ref[:-1]))


def test_block_method_on_a_downscaled_camera(gpu):
    video = _bgr_video(4, 960, 1504, k=6).to(gpu)
    fe = CameraFrontEnd((960, 1504), 3, 2, (256, 120, 240, 240))
    gray, ref = fe.process_batch_device(video), _restated(video, 2, fe.crop)
    assert torch.equal(gray, ref)
    bm = BlockMethod(240, 32, 8)
    for a, b in zip(bm.process_batch_device(gray[1:], gray[:-1]), bm.process_batch_device(ref[1:], ref[:-1])):
        assert torch.equal(a, b)


def test_graph_capture_front_end_and_fft_sequence(gpu):
    video = _bgr_video(6, 480, 752, k=7).to(gpu)
    fe = CameraFrontEnd((480, 752), 3, 1)
    fm = FftMethod(sample_point_size=64, frame_shape=(480, 752), grid=(8, 8), origin=(1, 1), stride=(98, 59))
    want = fm.process_sequence_device(fe.process_batch_device(video)).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fm.process_sequence_device(fe.process_batch_device(video))
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert _same(out, want)
    del g
    assert release_captured(fm) == 1


def test_refusals_leave_the_output_untouched(gpu):
    lib = _capi.load()
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 32, 64, 3), dtype=np.uint8)).to(gpu)
    out = torch.full((2, 10, 20), 0xA5, dtype=torch.uint8, device=gpu)
    good = _capi.FrontendConfig(64, 32, 3, 2, 2, 3, 20, 10)

    def call(cfg=good, src=None, ss=frames.stride(0), sp=frames.stride(1), n=2, dst=None, ds=out.stride(0), dp=out.stride(1)):
        src = frames.data_ptr() if src is None else src
        dst = out.data_ptr() if dst is None else dst
        return lib.mof_frontend_batch_device(C.byref(cfg), src, ss, sp, n, dst, ds, dp, None)

    refusals = [
        (dict(cfg=_capi.FrontendConfig(64, 32, 3, 3, 0, 0, 4, 4)), _capi.MOF_ERR_UNSUPPORTED),
        (dict(cfg=_capi.FrontendConfig(64, 32, 3, 2, 13, 0, 20, 10)), _capi.MOF_ERR_BAD_ARG),
        (dict(cfg=_capi.FrontendConfig(64, 32, 2, 2, 0, 0, 20, 10)), _capi.MOF_ERR_BAD_ARG),
        (dict(sp=64 * 3 - 1), _capi.MOF_ERR_BAD_ARG),
        (dict(dp=19), _capi.MOF_ERR_BAD_ARG),
        (dict(ds=199), _capi.MOF_ERR_BAD_ARG),
        (dict(n=-1), _capi.MOF_ERR_BAD_ARG),
        (dict(dst=0), _capi.MOF_ERR_BAD_ARG),
        (dict(src=0), _capi.MOF_ERR_BAD_ARG),
        (dict(dst=frames.data_ptr() + 100), _capi.MOF_ERR_BAD_ARG),  # overlaps the source
        (dict(src=out.data_ptr(), ss=0, sp=192, n=1), _capi.MOF_ERR_BAD_ARG),
    ]
    for kw, code in refusals:
        assert call(**kw) == code, kw
    assert call(n=0) == _capi.MOF_OK
    fe = CameraFrontEnd((32, 64), 3, 2, (2, 3, 20, 10))
    with pytest.raises(ValueError):
        fe.process_batch_device(frames[..., 0], out=out)  # mono frames to a BGR front end
    with pytest.raises(ValueError):
        fe.process_batch_device(frames, out=out[:, :, :19])
    with pytest.raises(MofError):
        CameraFrontEnd((32, 64), 3, 2, (2, 3, 40, 10))
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    # and the same call with good arguments writes it
    fe.process_batch_device(frames, out=out)
    assert np.array_equal(out.cpu().numpy(), frontend_ref.frontend(frames.cpu().numpy(), 2, (2, 3, 20, 10)))
