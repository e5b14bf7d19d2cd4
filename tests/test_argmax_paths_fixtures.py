"""tests/golden/argmax_paths_n*.npz (the inputs of tests/test_gpu_fft_argmax_paths.py) are what tests/golden/make_argmax_paths.py
builds, and the CPU oracle finds the arg-max of every pair of the sweep at the planted shift. No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_argmax_paths", os.path.join(GOLDEN, "make_argmax_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [64, 32])
def test_fixtures_are_what_their_maker_builds(n):
    mk = _maker()
    g = np.load(os.path.join(GOLDEN, f"argmax_paths_n{n}.npz"))
    cases = mk.build(n)
    assert g["cur"].dtype == np.uint8 and g["cur"].shape == (len(cases), n, n) and len(g["names"]) == len(cases)
    for key in ("want_shift", "want_shift_q", "want_quality"):  # recorded on the GPU (make_argmax_paths.py record)
        assert g[key].dtype == np.float64 and g[key].shape == (len(cases), 2), key
    for k, (name, cur, prev, planted) in enumerate(cases):
        assert str(g["names"][k]) == name and np.array_equal(g["cur"][k], cur) and np.array_equal(g["prev"][k], prev), name
        assert np.array_equal(g["planted"][k], planted if planted is not None else (np.nan, np.nan), equal_nan=True), name


@pytest.mark.parametrize("n", [64, 32])
def test_sweep_peaks_where_planted(n):
    mk = _maker()
    g = np.load(os.path.join(GOLDEN, f"argmax_paths_n{n}.npz"))
    sweep = [k for k in range(len(g["cur"])) if not np.isnan(g["planted"][k, 0])]
    assert len(sweep) == len(mk.DX[n]) * len(mk.DY[n]) == 90
    seen_x, seen_y = set(), set()
    for k in sweep:
        for prec in (32, 64):
            _, d = O.phase_correlate(g["cur"][k], g["prev"][k], prec)
            dx, dy = g["planted"][k]
            assert d["peak"] == (n // 2 + dx, n // 2 + dy), (str(g["names"][k]), prec, d["peak"])
            assert d["peak_value"] > 4 * abs(d["second_value"])  # one sharp sample
        seen_x.add(int(d["peak"][0]))
        seen_y.add(int(d["peak"][1]))
    # the shifted peak column walks through every wave's columns (n = 64: 8 column pairs per wave) and both halves of a packed pair;
    # the row (a lane of the last column stage holds the rows x + 8 k) through four lane rows x and through both halves of k
    assert {(x % (n // 2)) // 8 for x in seen_x} == set(range(n // 16)) and {x // (n // 2) for x in seen_x} == {0, 1}
    rows = {(y + n // 2) % n for y in seen_y}  # un-shifted
    assert len({y % 8 for y in rows}) >= 4 and {0, n // 16} <= {y // 8 for y in rows}
