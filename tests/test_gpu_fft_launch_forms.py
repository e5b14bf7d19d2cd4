"""Every front-end form each FFT launcher of csrc/ can select -- (gray | BGR8 | long-range) x (cv::phaseCorrelate's | the OpenCL
kernel's peak model) -- held to the CPU oracle on the route this process takes (tests/launch_form_cases.py has the cases).

The launchers pick a kernel instantiation from (downscale, channels, peak_model) through ONE dispatcher (csrc/pc_launch.hpp), and each
configure function raises the dynamic-LDS limit of the instantiations that dispatcher can return; a form that no test launches would
hide a wrong arm or a kernel left out of its configure list. The bars are those of tests/tolerances.py (check_patch), nothing new.
A wrong arm must FAIL here rather than pass by accident: before a case touches the GPU it is asserted on the CPU that the oracle's
answer for the neighbouring forms on the same bytes lies more than two bars from the expected one on at least half of the patches
(launch_form_cases.assert_forms_apart; test_forms_are_told_apart runs the same check without a GPU).

By default: the cases of the default route. In a child process of test_gpu_fft_quality_forms.py, where a knob has changed the route,
MOF_LAUNCH_FORM_CASES = 'name=kernel_variant,...' names the cases and the variant the knob must give them."""
import os

import numpy as np
import pytest

import launch_form_cases as L


def _selected():
    v = os.environ.get("MOF_LAUNCH_FORM_CASES")
    if v is None:
        return [(name, c.variant) for name, c in L.CASES.items()]
    return [tuple(item.split("=")) for item in v.split(",") if item]


@pytest.mark.parametrize("name", list(L.CASES))
def test_forms_are_told_apart(name):
    """CPU only: the inputs of every case separate its form from the neighbouring ones by more than two bars on at least half of the
    patches, and the case has an answer on every patch (no gated or degenerate patch hides behind a NaN)"""
    case = L.CASES[name]
    apart = L.assert_forms_apart(case)
    assert np.isfinite(case.want[0]).all() and np.isfinite(case.want[1]).all(), name
    assert case.channels == 1 or len(apart) >= 2, (name, apart)
    print(f"{name}: patches apart of {case.want[0].shape[0] * case.want[0].shape[1]}: {apart}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", _selected())
def test_launch_form_on_its_route(request, name, variant):
    """One case through the public entry that expresses its form, on the route this process takes (kernel_variant from the
    parametrisation), every patch against both oracles; the quality entry of the same call must leave the shifts' bits alone (the
    same kernel with the quality pointer set). The wrong-form separation is asserted on the CPU first; only then is the device asked
    for (the `gpu` fixture)."""
    case = L.CASES[name]
    print(f"{name}: patches apart on the CPU: {L.assert_forms_apart(case)}")
    gpu = request.getfixturevalue("gpu")
    import torch

    fm = L.engine(case)
    print(f"form {name}: kernel_variant {fm.kernel_variant}")
    assert fm.kernel_variant == variant, (name, fm.kernel_variant, variant)
    got = L.run(case, fm, gpu)
    with_q, quality = L.run(case, fm, gpu, return_quality=True)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    pinned = L.check(case, got, f"{name} ({fm.kernel_variant})")
    assert pinned == got.shape[0] * got.shape[1], (name, pinned)
    assert np.array_equal(got.view(np.uint64), with_q.cpu().numpy().view(np.uint64)) and torch.isfinite(quality).all(), name


@pytest.mark.gpu
def test_rejected_combinations(gpu):
    """What the form dispatch has no kernel for is refused by the public entries that can express it, with the status they always gave:
    BGR8 frames in the long-range mode, channel counts other than 1 and 3, a long_range flag other than 0 and 1 (MOF_ERR_BAD_ARG from
    the _q entries, before anything is launched: the outputs stay untouched); a peak model other than the two (MOF_ERR_BAD_ARG at
    create); the OpenCL model at sizes the reference cannot plan under it -- 136 = 8 x 17, the padded 11 and 74 -- (MOF_ERR_UNSUPPORTED
    at create); the long-range mode outside the reference tiling (MOF_ERR_UNSUPPORTED). The engine works afterwards."""
    import torch

    from mrs_optic_flow_amd import FftMethod, _capi
    from mrs_optic_flow_amd.engine import PEAK_OCL

    case = L.CASES["k1-64-lr-cv"]  # 256 x 256 frames in the reference tiling: a geometry with a long-range form
    fm = L.engine(case)
    lib = fm._lib
    n_lr = lib.mof_fft_long_range_patches(fm._h)
    assert n_lr == 1
    h, w = case.shape
    bgr = torch.zeros((1, h, w, 3), dtype=torch.uint8, device=gpu)
    gray = torch.from_numpy(np.array(case.cur)).to(gpu)
    prev = torch.from_numpy(np.array(case.prev)).to(gpu)
    out = torch.full((1, fm.n_patches, 2), 7.0, dtype=torch.float64, device=gpu)
    q = torch.full((1, fm.n_patches, 2), 7.0, dtype=torch.float64, device=gpu)

    def batch_q(t, channels, long_range):
        return lib.mof_fft_process_batch_device_q(fm._h, t.data_ptr(), t.stride(0), t.data_ptr(), t.stride(0), t.stride(1), 1, channels, long_range,
                                                  out.data_ptr(), q.data_ptr(), None)

    assert batch_q(bgr, 3, 1) == _capi.MOF_ERR_BAD_ARG
    for channels in (0, 2, 4):
        assert batch_q(bgr, channels, 0) == _capi.MOF_ERR_BAD_ARG, channels
    for long_range in (-1, 2, 4):
        assert batch_q(gray, 1, long_range) == _capi.MOF_ERR_BAD_ARG, long_range
    video = torch.zeros((3, h, w, 3), dtype=torch.uint8, device=gpu)
    for channels in (0, 2, 4):
        rc = lib.mof_fft_process_sequence_device_q(fm._h, video.data_ptr(), video.stride(0), video.stride(1), 3, channels, out.data_ptr(),
                                                   q.data_ptr(), None)
        assert rc == _capi.MOF_ERR_BAD_ARG, channels
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((q == 7.0).all()), "a refused call must not launch"

    def create_status(**kw):
        with pytest.raises(_capi.MofError) as e:
            FftMethod(max_px_speed=L.SPEED, **kw)
        return e.value.code

    assert create_status(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1), peak_model=2) == _capi.MOF_ERR_BAD_ARG
    assert create_status(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1), peak_model=-1) == _capi.MOF_ERR_BAD_ARG
    for n in (136, 11, 74):
        assert create_status(sample_point_size=n, frame_shape=(n, n), grid=(1, 1), peak_model=PEAK_OCL) == _capi.MOF_ERR_UNSUPPORTED, n
    off = FftMethod(sample_point_size=64, max_px_speed=L.SPEED, frame_shape=(h + 1, w + 1), grid=(4, 4), origin=(1, 1))
    assert lib.mof_fft_long_range_patches(off._h) == _capi.MOF_ERR_UNSUPPORTED
    with pytest.raises(_capi.MofError) as e:
        off.process_long_range_batch_device(torch.zeros((1, h + 1, w + 1), dtype=torch.uint8, device=gpu), torch.zeros((1, h + 1, w + 1), dtype=torch.uint8, device=gpu))
    assert e.value.code == _capi.MOF_ERR_UNSUPPORTED
    # ... and the engine still answers: the case's own pair in the long-range mode
    got = fm.process_long_range_batch_device(gray, prev).cpu().numpy()
    assert L.check(case, got, "after the refused calls") == 1
