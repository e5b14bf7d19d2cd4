"""CPU tests of the inputs of the response-gate tests (tests/gate_cases.py): for every batch test_gpu_fft_gate.py uses, the f64 and the f32
oracle each put the matched and the unrelated patches at least 1000 quality bars (360 d, quality_cases.Batch.bar) apart, so a kernel
within its bar cannot move a patch across the batch's threshold -- the midpoint of the f64 oracle's gap -- and the gated set the GPU tests
expect is a property of the input, not of a kernel. Prints every batch's figures (run with -s). No GPU."""
import numpy as np
import pytest

import gate_cases as G


@pytest.mark.parametrize("name", sorted(G.BATCHES))
def test_classes_are_a_thousand_bars_apart(name):
    g = G.BATCHES[name]()
    assert g.unrelated.any() and (~g.unrelated).any(), name
    for precision in (64, 32):
        matched, unrel = g.gap(precision)
        print(f"{g.name} f{precision}: smallest matched response {matched:.4f}, largest unrelated {unrel:.4f}, gap {matched - unrel:.4f} = "
              f"{(matched - unrel) / g.b.bar:.0f} bars of {g.b.bar:.3e}; v = {g.v:.6f}")
        assert matched - unrel >= G.GAP_BARS * g.b.bar, (name, precision, matched, unrel, g.b.bar)
        r = (g.b.want if precision == 64 else g.b.want32)[..., 0]
        assert np.array_equal(~(r >= g.v), g.unrelated), (name, precision)
    assert np.array_equal(g.gated, g.unrelated) and g.lo < g.v < g.hi


def test_the_placed_patches_are_where_the_tests_say():
    """flat indices 0, 255, 256, 319 of the 320 patches; one patch per pair at k mod 6 on the 3 x 2 grid; frame 2 of the videos"""
    assert np.flatnonzero(G.index320().unrelated.ravel()).tolist() == [0, 255, 256, 319]
    assert [np.flatnonzero(row).tolist() for row in G.grid7().unrelated] == [[k % 6] for k in range(7)]
    assert G.video(64).unrelated.all(axis=1).tolist() == [False, True, True, False]
    assert int(G.rt480().unrelated.sum()) == 5 and int(G.passes200().unrelated.sum()) == 7


def test_constant_patch_is_below_every_threshold():
    """a 64 x 64 texture against a constant patch under cv::phaseCorrelate's model: a finite shift the validity rule passes, response
    far below the threshold of the batch it joins (test_gpu_fft_gate.py::test_constant_patch_n64)"""
    import oracle_lib as O
    import quality_cases as Q

    tex = np.random.default_rng(11).integers(0, 256, (64, 64), dtype=np.uint8)
    q, _, shifts = Q.oracle_quality(tex[None], np.full((1, 64, 64), 81, np.uint8), 64)
    print(f"constant patch: response {q[0, 0, 0]:.3e}, shift {shifts[0, 0].tolist()}, threshold {G.family(64).v:.4f}")
    assert np.isfinite(shifts).all() and 0.0 <= q[0, 0, 0] < 1e-6 < G.family(64).v
