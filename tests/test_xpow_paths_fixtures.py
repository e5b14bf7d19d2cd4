"""tests/golden/xpow_paths_*.npz (the inputs of tests/test_gpu_fft_xpow_paths.py) are what tests/golden/make_xpow_paths.py builds, and the
oracle outputs frozen in them are what the oracle gives today. No GPU."""
import importlib.util
import os

import numpy as np
import pytest

import oracle_lib as O

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _maker():
    spec = importlib.util.spec_from_file_location("make_xpow_paths", os.path.join(GOLDEN, "make_xpow_paths.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("n", [64, 32])
def test_fixtures_are_what_their_maker_builds(n):
    mk = _maker()
    lay = O.fft_layout(n, n, n, 1, 1)
    built = mk.build(n)
    assert sorted(built) == ["main", "mixed", "one_wave", "tile"]
    for name, pairs in built.items():
        g = np.load(os.path.join(GOLDEN, f"xpow_paths_{name}_n{n}.npz"))
        assert g["cur"].dtype == np.uint8 and g["cur"].shape == (len(mk.SHIFTS), n, n)
        for k, (cur, prev) in enumerate(pairs):
            assert np.array_equal(g["cur"][k], cur) and np.array_equal(g["prev"][k], prev), (name, k)
            for prec, key, atol in ((64, "oracle64", 1e-9), (32, "oracle32", 1e-5)):  # (the bars of test_golden_vectors_reproduce)
                want, _ = O.fft_process(g["cur"][k], g["prev"][k], lay, prec)
                assert np.allclose(g[key][k], want, rtol=0, atol=atol), (name, k, prec)
            # the oracles alone meet the strict rule with no relaxation: closer than 2e-5 px to each other
            assert np.abs(g["oracle64"][k] - g["oracle32"][k]).max() <= 2e-5
