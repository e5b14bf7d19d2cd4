"""No-GPU tests of the OpenCL peak model's (MOF_PEAK_OCL) size range: every even 5-smooth patch size up to 960 -- the sizes the
reference's OpenCL branch can plan -- passes validation, so create only stops at the missing device; every other size is refused
before any device use."""
import ctypes as C

import pytest

from mrs_optic_flow_amd import _capi


def _create(n, peak_model=1):
    lib = _capi.load()
    fs = n + 4
    cfg = _capi.FftConfig(fs, fs, n, 1, 1, 2, 1, n, n, 80.0, 0, peak_model, 55)
    h = C.c_void_p()
    rc = lib.mof_fft_create(C.byref(cfg), C.byref(h))
    if h:
        lib.mof_fft_destroy(h)
    return rc, lib.mof_last_error()


@pytest.mark.parametrize("n", [160, 240, 480, 144, 200, 750, 810, 960])
def test_ocl_model_accepts_large_even_5_smooth_patches(n):
    rc, msg = _create(n)
    assert rc in (_capi.MOF_ERR_NO_DEVICE, _capi.MOF_OK), (n, rc, msg)


@pytest.mark.parametrize("n", [138, 145, 470, 1000])
def test_ocl_model_refuses_what_the_reference_cannot_plan(n):
    # 138 = 2 * 3 * 23 and 470 = 2 * 5 * 47 are not 5-smooth, 145 is odd, 1000 is beyond the planned transforms
    rc, msg = _create(n)
    assert rc == _capi.MOF_ERR_UNSUPPORTED, (n, rc, msg)
    assert (b"960" in msg) if n == 1000 else (b"MOF_PEAK_OCL" in msg), msg
    # the cv::phaseCorrelate model pads 138, 145 and 470 (to 144, 150 and 480) and runs them
    rc, msg = _create(n, peak_model=0)
    if n == 1000:
        assert rc == _capi.MOF_ERR_UNSUPPORTED, msg
    else:
        assert rc in (_capi.MOF_ERR_NO_DEVICE, _capi.MOF_OK), (n, rc, msg)
