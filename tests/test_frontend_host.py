"""No-GPU tests of the camera front end (include/mof.h, mof_frontend_*): the node's rectangle, the argument checks, the refusal
without a device, and the numpy restatement the GPU tests compare with, anchored to the oracle."""
import ctypes as C

import numpy as np
import pytest

import frontend_ref
import oracle_lib
from mrs_optic_flow_amd import CameraFrontEnd, MofError, _capi

OK, BAD, UNSUP = _capi.MOF_OK, _capi.MOF_ERR_BAD_ARG, _capi.MOF_ERR_UNSUPPORTED


def _reference(w, h, ch, s, fs, cx):
    cfg = _capi.FrontendConfig()
    rc = _capi.load().mof_frontend_config_reference(C.byref(cfg), w, h, ch, s, fs, cx)
    return rc, (cfg.crop_x, cfg.crop_y, cfg.crop_width, cfg.crop_height)


def test_reference_rectangle_follows_the_node():
    # optic_flow.cpp:867-869, :1604, :1611-1614: fs' = fs / s, xi = (int)cx - fs'/2, yi = (H/s)/2 - fs'/2
    assert _reference(752, 480, 3, 1, 480, 376.6) == (OK, (136, 0, 480, 480))
    assert _reference(1504, 960, 3, 2, 480, 376.0) == (OK, (256, 120, 240, 240))
    assert _reference(752, 480, 1, 1, 240, 300.9) == (OK, (180, 120, 240, 240))  # (int)cx truncates
    # the node's out-of-range crop: the scaled image is 376 wide, the crop centred on the UNSCALED cx_ ends at 496
    rc, _ = _reference(752, 480, 3, 2, 480, 376.0)
    assert rc == BAD
    assert "cx_" in _capi.load().mof_last_error().decode()
    # 752 % 3 != 0: the ratio is checked before the crop
    assert _reference(752, 480, 3, 3, 480, 376.0)[0] == UNSUP
    assert _reference(752, 480, 3, 0, 480, 376.0)[0] == BAD
    assert _reference(752, 480, 2, 1, 480, 376.0)[0] == BAD
    assert _reference(752, 480, 3, 1, 480, 100.0)[0] == BAD  # xi < 0
    assert _reference(752, 480, 3, 1, 480, float("nan"))[0] == BAD
    assert _capi.load().mof_frontend_config_reference(None, 752, 480, 3, 1, 480, 376.0) == BAD


def test_validate_codes():
    lib = _capi.load()

    def v(*fields):
        cfg = _capi.FrontendConfig(*fields)
        return lib.mof_frontend_validate(C.byref(cfg))

    assert v(752, 480, 3, 1, 136, 0, 480, 480) == OK
    assert v(1920, 1080, 1, 4, 120, 15, 240, 240) == OK
    assert v(1920, 1080, 1, 4, 0, 0, 480, 270) == OK  # the whole downscaled image
    assert v(1920, 1080, 1, 4, 0, 0, 480, 271) == BAD
    assert v(1920, 1080, 1, 4, 1, 0, 480, 270) == BAD
    assert v(752, 480, 3, 1, -1, 0, 10, 10) == BAD
    assert v(752, 480, 3, 1, 0, 0, 0, 10) == BAD
    assert v(752, 480, 2, 1, 0, 0, 10, 10) == BAD
    assert v(752, 480, 3, 0, 0, 0, 10, 10) == BAD
    assert v(752, 480, 3, -2, 0, 0, 10, 10) == BAD
    assert v(0, 480, 3, 1, 0, 0, 10, 10) == BAD
    assert v(752, 480, 3, 3, 0, 0, 10, 10) == UNSUP  # 752 % 3
    assert v(750, 481, 1, 3, 0, 0, 10, 10) == UNSUP  # 481 % 3
    assert v(752, 480, 3, 5, 0, 0, 10, 10) == UNSUP
    assert lib.mof_frontend_validate(None) == BAD


def test_batch_argument_checks_launch_nothing():
    """Refusals happen before any device is touched (fake addresses, never dereferenced)."""
    lib = _capi.load()
    cfg = _capi.FrontendConfig(64, 32, 3, 2, 2, 3, 20, 10)
    src, dst = 1 << 32, 1 << 36
    fb = 32 * 64 * 3

    def call(s=src, ss=fb, sp=64 * 3, n=2, d=dst, ds=10 * 20, dp=20, c=cfg):
        return lib.mof_frontend_batch_device(C.byref(c) if c is not None else None, s, ss, sp, n, d, ds, dp, None)

    assert call(n=0, s=None, d=None) == OK  # an empty batch is a no-op
    assert call(n=-1) == BAD
    assert call(s=None) == BAD
    assert call(d=None) == BAD
    assert call(sp=64 * 3 - 1) == BAD  # pitch below 3 * W
    assert call(dp=19) == BAD  # pitch below the crop width
    assert call(ds=10 * 20 - 1) == BAD  # output crops overlap each other
    assert call(d=src + fb) == BAD  # inside frame 1
    assert call(s=dst + 100) == BAD
    assert call(c=None) == BAD
    assert call(c=_capi.FrontendConfig(64, 32, 3, 3, 0, 0, 4, 4)) == UNSUP
    assert call(c=_capi.FrontendConfig(64, 32, 3, 2, 30, 0, 4, 4)) == BAD  # crop outside the 32 x 16 image


def test_no_device_without_a_gpu():
    lib = _capi.load()
    if lib.mof_device_count() > 0:
        pytest.skip("a HIP device is present")
    cfg = _capi.FrontendConfig(64, 32, 1, 1, 0, 0, 64, 32)
    assert lib.mof_frontend_batch_device(C.byref(cfg), 1 << 32, 2048, 64, 1, 1 << 36, 2048, 64, None) == _capi.MOF_ERR_NO_DEVICE


def test_python_handle():
    fe = CameraFrontEnd.reference((480, 752), 3, 1, 480, 376.6)
    assert fe.crop == (136, 0, 480, 480) and fe.out_shape == (480, 480)
    fe2 = CameraFrontEnd.reference((960, 1504), 3, 2, 480, 376.0)
    assert fe2.crop == (256, 120, 240, 240) and fe2.out_shape == (240, 240)
    assert CameraFrontEnd((1080, 1920), 1, 4).out_shape == (270, 480)
    assert CameraFrontEnd((1080, 1920), 1, 4, (120, 15, 240, 240)).out_shape == (240, 240)
    with pytest.raises(MofError) as e:
        CameraFrontEnd.reference((480, 752), 3, 2, 480, 376.0)
    assert e.value.code == BAD and "cx_" in str(e.value)
    with pytest.raises(MofError) as e:
        CameraFrontEnd((480, 752), 3, 3)
    assert e.value.code == UNSUP
    with pytest.raises(MofError) as e:
        CameraFrontEnd((480, 752), 3, 1, (700, 0, 100, 10))
    assert e.value.code == BAD


def test_restatement_is_the_oracle_quarter():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (2, 96, 136), dtype=np.uint8)
    got = frontend_ref.frontend(frames, 4)
    for k in range(2):
        assert np.array_equal(got[k], oracle_lib.resize_quarter(frames[k]))


def test_restatement_is_the_oracle_gray():
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    got = frontend_ref.frontend(frames, 1)
    for k in range(2):
        assert np.array_equal(got[k], oracle_lib.rgb2gray(frames[k]))
    # a crop of the s = 1 image is the crop of the converted frame; mono at s = 1 is the crop itself
    assert np.array_equal(frontend_ref.frontend(frames, 1, (5, 3, 11, 7))[0], oracle_lib.rgb2gray(frames[0])[3:10, 5:16])
    assert np.array_equal(frontend_ref.frontend(frames[..., 1], 1, (5, 3, 11, 7)), frames[:, 3:10, 5:16, 1])


def test_restatement_even_factor_forms():
    """s = 2 is cv::resize's INTER_AREA fast path (the 2 x 2 mean) -- the even closed form at s = 2 -- and odd s picks the centre
    pixel of each s x s cell; checked against a direct per-pixel loop."""
    rng = np.random.default_rng(13)
    img = rng.integers(0, 256, (1, 12, 18), dtype=np.uint8)
    a2 = frontend_ref.frontend(img, 2)[0]
    want = (img[0, 0::2, 0::2].astype(int) + img[0, 0::2, 1::2] + img[0, 1::2, 0::2] + img[0, 1::2, 1::2] + 2) >> 2
    assert np.array_equal(a2, want)
    a3 = frontend_ref.frontend(img, 3)[0]
    assert np.array_equal(a3, img[0, 1::3, 1::3])
    a6 = frontend_ref.frontend(img, 6)[0]
    want6 = (img[0, 2::6, 2::6].astype(int) + img[0, 2::6, 3::6] + img[0, 3::6, 2::6] + img[0, 3::6, 3::6] + 2) >> 2
    assert np.array_equal(a6, want6)
