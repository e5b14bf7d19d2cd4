"""CPU only: the cases of test_gpu_fft_route_classes.py (tests/route_cases.py) stand for what they claim and are ordinary inputs, so that
the GPU test's plain 1e-4 px bar against both oracles hides nothing:
  * each case's (peak model, patch size) has the route class it stands for in tests/golden/fft_route_table.txt, and the cases cover
    every class of the default table,
  * the f32 and the f64 oracle are within 2e-5 px of each other on every patch (tolerances.F32_LIMITED_FROM: the fast path's condition),
    with an answer near the planted shift everywhere,
  * tests/conditioning.py, from the pixels alone, finds no mechanism that relaxes or unpins a patch: no exact-zero bin, no cancelling
    centroid window, independent f32 transforms within 2e-5 px of the f64 pipeline, and tolerances.allowance says `pinned`."""
import numpy as np
import pytest

import conditioning
import route_cases as R
import tolerances


def test_cases_cover_every_class_of_the_default_table():
    table = R.default_table()
    assert len(table) == 2 * 999
    classes = {(model, R.route_class(row)) for (model, _), row in table.items() if row is not None}
    assert len(classes) == 16
    assert {(model, klass) for (model, _), klass in R.CASES.items()} == classes
    for (model, n), klass in R.CASES.items():
        assert R.route_class(table[(model, n)]) == klass, (model, n, table[(model, n)])


@pytest.mark.parametrize("model,n", list(R.CASES))
def test_case_is_pinned_by_its_inputs(model, n):
    c = R.case(model, n)
    dd = np.abs(c.want64 - c.want32).max(axis=-1)  # [pair, patch]
    print(f"model {model} n {n}: oracle distance {dd.max():.2e} px, f64 answers {c.want64.round(3).tolist()}")
    assert np.isfinite(c.want64).all() and np.isfinite(c.want32).all()
    assert dd.max() <= tolerances.F32_LIMITED_FROM, dd
    planted = np.array([[3, -2], [-5, 3]], np.float64)[:, None, :]
    # (a crop is no circular shift and a padded patch has edges: the centroid is biased by a fraction of a pixel, the peak is the planted one)
    assert np.abs(c.want64 - planted).max() < 1.0, c.want64
    for k in range(2):
        for p in range(2):
            info = conditioning.analyse(*c.patch_pixels(k, p))
            allow, unpinned = tolerances.allowance(info, float(dd[k, p]))
            print(f"  pair {k} patch {p}: {info['mechanism']}, spread {info['spread_px']:.2e} px, cancellation {info['cancellation']:.2f}")
            assert not unpinned and info["zero_bins"] == 0 and info["cancellation"] <= conditioning.CANCEL_FROM, (k, p, info)
            assert info["spread_px"] <= tolerances.F32_LIMITED_FROM and allow <= tolerances.SPREAD_FACTOR * tolerances.F32_LIMITED_FROM, (k, p, info, allow)
