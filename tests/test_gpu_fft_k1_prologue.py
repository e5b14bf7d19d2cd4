"""What a wave of K1 runs before its first butterfly -- the kernel arguments, the two 16-byte lane loads and their addresses, the
constant-patch test, the byte extraction of the first row stage (csrc/pc_kernel.hip, csrc/pc_passes3.hpp) -- was rewritten without
touching the transform's arithmetic: every result keeps its bits. The fixture tests/golden/k1_prologue.npz (made by
tests/golden/make_k1_prologue.py; the cases and what each is for: tests/k1_prologue_cases.py) was recorded ONCE on the GPU from the
commit before that change; every float64 of the shifts, through the default entry and the _q entry, and of the quality must come out
with the same bits."""
import os

import numpy as np
import pytest
import torch

import k1_prologue_cases as K
from mrs_optic_flow_amd import FftMethod

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "k1_prologue.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", [name for name, _ in K.CASES])
def test_same_bits_as_recorded(gpu, golden, name):
    got = dict(K.CASES)[name](golden, gpu)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(got) and "shift" in keys and "quality" in keys, (keys, sorted(got))
    for key in keys:
        have, want = got[key], golden[f"{name}/{key}"]
        assert have.shape == want.shape, (name, key, have.shape, want.shape)
        bad = np.argwhere((_bits(have) != _bits(want)).any(axis=-1))
        for idx in bad[:8]:
            print(f"k1 prologue [{name}] {key} {idx.tolist()}: got {have[tuple(idx)].tolist()} recorded {want[tuple(idx)].tolist()}")
        assert len(bad) == 0, (name, key, bad[:8].tolist(), len(bad))


def test_constant_classes_are_what_they_claim(golden):
    """the record is about the classes the case names (no GPU): which slots hold a constant patch, and that the near-constant ones pass the
    pre-test (every lane's dwords 0 and 1 equal) without being constant"""
    cur, prev = golden["const_cur"], golden["const_prev"]

    def patch(a, slot):
        k, j, i = slot // 4, (slot % 4) // 2, slot % 2
        return a[k, 1 + 70 * j:1 + 70 * j + 64, 80 * i:80 * i + 64]

    def constant(p):
        return bool((p == p[0, 0]).all())

    def pretest_maybe(p):  # in every wave's 16 rows
        d = p.reshape(64, 4, 4, 4)
        return [bool((d[16 * w:16 * w + 16, :, 0] == d[16 * w:16 * w + 16, :, 1]).all()) for w in range(4)]

    assert [s for s in range(12) if constant(patch(cur, s))] == [0, 2, 3]
    assert [s for s in range(12) if constant(patch(prev, s))] == [1, 2, 3]
    assert pretest_maybe(patch(cur, 4)) == [True, False, False, False] and pretest_maybe(patch(prev, 5)) == [False, False, True, False]
    for a, slots in ((cur, (6, 8, 10)), (prev, (7, 9))):
        for s in slots:
            assert all(pretest_maybe(patch(a, s))) and not constant(patch(a, s)), s


def test_row_pitch_of_16_mib_is_refused(gpu):
    """The one-patch forms add ONE 32-bit lane offset, row * pitch + column bytes from a 24-bit multiply, to a scalar patch base: every
    field launch holds the pitch below 2^24 (csrc/mof_kernels.h, PC_MAX_PITCH) and answers MOF_ERR_BAD_ARG beyond it -- before anything is
    launched, so the pointers here are never read."""
    from mrs_optic_flow_amd import _capi

    out = torch.empty((1, 4, 2), dtype=torch.float64, device=gpu)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for n in (64, 32, 128, 60):  # one bound for every kernel family: the tuned sizes and a planned one
        fm = FftMethod(sample_point_size=n, frame_shape=(2 * n, 2 * n), grid=(2, 2))
        frames = torch.zeros((1, 2 * n, 2 * n), dtype=torch.uint8, device=gpu)
        rc = fm._lib.mof_fft_process_batch_device(fm._h, frames.data_ptr(), 0, frames.data_ptr(), 0, 1 << 24, 1, out.data_ptr(), stream)
        assert rc == _capi.MOF_ERR_BAD_ARG, (n, rc)
        assert "pitch" in fm._lib.mof_last_error().decode()
        # (the engine is as usable as before)
        assert tuple(fm.process_batch_device(frames, frames).shape) == (1, 4, 2)


def test_launch_split_after_65535_pairs(gpu, golden):
    """One workgroup per patch on a 3-D grid, no `p < total` guard: a batch of 65 540 pairs of one 64 x 64 patch goes out in two launches
    (pc_split_pairs), the second of 5 pairs. Pair k carries the recorded bits of pair k mod 8 of the first period."""
    fm = FftMethod(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1))
    assert fm.kernel_variant == "stockham"
    cur, prev = K.split_batch(golden, gpu)
    assert cur.shape[0] == K.SPLIT_PAIRS
    shifts, quality = fm.process_batch_device(cur, prev, return_quality=True)
    plain = fm.process_batch_device(cur, prev)
    k = np.arange(K.SPLIT_PAIRS) % K.SPLIT_PERIOD
    for what, have, want in (("default entry", plain, golden["split period/shift"]), ("_q entry, shift", shifts, golden["split period/shift_q"]),
                             ("_q entry, quality", quality, golden["split period/quality"])):
        off = np.argwhere((_bits(have.cpu().numpy()) != _bits(want)[k]).any(axis=(1, 2))).ravel()
        print(f"split, {what}: {len(k) - off.size} of {len(k)} pairs carry the recorded bits of their pair of the first period")
        assert off.size == 0, (what, off[:4].tolist(), int(off.size))
