"""CPU tests of the per-patch correlation quality (include/mof.h, the *_q entries): the five entries exist and refuse a null engine,
and the oracle facts the GPU bars of test_gpu_fft_quality.py rest on hold for every batch that file uses (recomputed here from the
same builders, tests/quality_cases.py, so they cannot rot)."""
import numpy as np
import pytest

import quality_cases as Q
from mrs_optic_flow_amd import _capi

# the f32 and the f64 oracle of cv::phaseCorrelate's model agree on (response, peak / M^2) within 1.7e-7 on these batches
D_MAX = 2e-7
# the OpenCL model's response is a FLOAT running sum of up to 49 positive window values in its f32 oracle (oracle/pc_ref_impl.h:368-377):
# each of the 49 additions rounds by at most half an ulp of a partial sum below the largest response of these batches (1.1 < 2)
D_MAX_OCL = 49 * 2.0 ** -24


def test_q_entries_refuse_a_null_engine():
    lib = _capi.load()
    nil = None
    assert lib.mof_fft_process_q(nil, nil, 0, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_fft_process_long_range_q(nil, nil, 0, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_fft_process_batch_device_q(nil, nil, 0, nil, 0, 0, 1, 1, 0, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    # (a null engine is reported before the channel / long-range combination the kernels refuse)
    assert lib.mof_fft_process_batch_device_q(nil, nil, 0, nil, 0, 0, 1, 3, 1, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_fft_process_sequence_device_q(nil, nil, 0, 0, 2, 1, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_fft_process_batch_host_q(nil, nil, 0, nil, 0, 0, 1, nil, nil) == _capi.MOF_ERR_NOT_INIT


@pytest.mark.parametrize("name", sorted(Q.BATCHES))
def test_batches_are_clear_peak_and_the_oracles_agree(name):
    """Every pair of every GPU batch has ONE peak (the runner-up outside the window stays under half of it in the f64 oracle: the first
    maximum cannot flip between two precisions), and the two oracles' mutual distance -- what the GPU bar is a multiple of -- is the
    f32 format's."""
    batch = Q.BATCHES[name]()
    assert batch.want.shape[0] == len(batch.cur) and np.isfinite(batch.want).all()
    assert (batch.ratio < 0.5).all(), (batch.name, np.argwhere(batch.ratio >= 0.5).tolist(), float(batch.ratio.max()))
    print(f"{batch.name}: d = {batch.d_slot[0]:.2e} (response), {batch.d_slot[1]:.2e} (peak); second / peak <= {batch.ratio.max():.3f}")
    assert batch.d <= (D_MAX_OCL if batch.ocl else D_MAX), (batch.name, batch.d_slot.tolist())


def test_circular_batches_carry_their_gated_pairs():
    """11 of the 36 circular-shift pairs are gated (a -n/2 component): their shift is NaN, their oracle quality finite"""
    for n, _ in Q.CIRCULAR_SIZES:
        b = Q.circular(n)
        assert int(np.isnan(b.shifts[:, 0, 0]).sum()) == 11 and np.isfinite(b.want).all()
