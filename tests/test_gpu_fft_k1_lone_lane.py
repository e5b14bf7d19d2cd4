"""How the wave that holds the maximum of a 64 x 64 surface comes by its pair under cv::phaseCorrelate's peak model (csrc/pc_kernel.hip,
holder_pair): every lane takes its index from an equality mask over its 16 values in the fixed order of their shifted index
(csrc/pc_passes.hpp, col_pass_inv_index_mask), and where ONE lane of the wave is at the maximum the wave reads that lane's own (value,
index) with two v_readlane instead of folding 64 pairs; two lanes at the maximum, a +0 beside a -0 and the flat surfaces keep the fold.
Either way the pair is the one the fold returned before (csrc/pc_argmax.hpp; tests/cpp/test_argmax_lone.cpp holds the rule to the fold on
the host), so every result keeps its bits. The fixture tests/golden/k1_lone_lane.npz (made by tests/golden/make_k1_lone_lane.py; the cases
and what each is for: tests/k1_lone_lane_cases.py) was recorded ONCE on the GPU from the library of the commit before that change; every
float64 of the shifts, through the default entry (quality null) and the _q entry, and of the quality must come out with the same bits."""
import os

import numpy as np
import pytest

import k1_lone_lane_cases as L

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "k1_lone_lane.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [name for name, _ in L.CASES])
def test_same_bits_as_recorded(gpu, golden, name):
    got = dict(L.CASES)[name](golden, gpu)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(got) and keys == ["quality", "shift", "shift_q"], (keys, sorted(got))
    for key in keys:
        have, want = got[key], golden[f"{name}/{key}"]
        assert have.shape == want.shape, (name, key, have.shape, want.shape)
        bad = np.argwhere((_bits(have) != _bits(want)).any(axis=-1))
        for idx in bad[:8]:
            print(f"k1 lone lane [{name}] {key} {idx.tolist()}: got {have[tuple(idx)].tolist()} recorded {want[tuple(idx)].tolist()}")
        assert len(bad) == 0, (name, key, bad[:8].tolist(), len(bad))


def test_inputs_are_what_the_cases_name(golden):
    """the recorded inputs are the generators' own, the tie cases have their exact periods, and the recorded results say that the lone
    peaks fall where the cases put them (numpy, no GPU)"""
    made = L.make_inputs()
    assert sorted(made) == sorted(k for k in golden if "/" not in k)
    for k, a in made.items():
        assert a.dtype == golden[k].dtype and np.array_equal(a, golden[k]), k
    L.check_inputs(golden)
    # a lone lane in each wave, both column halves, both halves of the lane's order: wave = (un-shifted peak column % 32) // 8; the
    # un-shifted peak is the rounded shift mod 64 (the centroid lies within a pixel of the first maximum)
    s = golden["lone lane in each wave/shift"][:, 0]
    assert not np.isnan(s).any()
    col, row = np.rint(s[:, 0]).astype(int) % L.N, np.rint(s[:, 1]).astype(int) % L.N
    seen = {(int(c % 32) // 8, bool(c >= 32), bool(r >= 32)) for c, r in zip(col, row)}
    assert seen == {(w, ch, rh) for w in range(4) for ch in (False, True) for rh in (False, True)}, sorted(seen)
    # flat surfaces answer as they always did: a constant patch 9 c / (9 c + eps) - 32 in both components, the all-zero pair (-32, -32)
    st = golden["several holders/shift"][:, 0]
    assert np.allclose(st[:3], -31.0, rtol=0, atol=1e-4) and st[3].tolist() == [-32.0, -32.0], st.tolist()
