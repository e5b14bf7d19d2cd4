"""GPU test of the cross-lane helpers every peak tail ends in (csrc/pc_common.hpp: lane_xor, wave_best, wave_sum3): the library's own
self-test (csrc/wave_selftest.hip) -- one launch of one wave that compares lane_xor<OFF> with __shfl_xor for every level on 32- and
64-bit patterns, wave_best with a serial scan (distinct values, ties within and across the 32-lane halves, all -inf, one NaN lane,
all NaN) and wave_sum3 bit for bit with the __shfl_xor butterfly on 25 and 49 non-zero lanes -- counts no mismatch."""
import ctypes

import pytest

from mrs_optic_flow_amd import _capi

pytestmark = pytest.mark.gpu


def test_wave_ops_selftest_counts_no_mismatch(gpu):
    fn = _capi.load().mof_selftest_wave_ops  # (not in include/mof.h: no entry in _capi.SYMBOLS)
    fn.restype, fn.argtypes = ctypes.c_int, []
    assert fn() == 0
