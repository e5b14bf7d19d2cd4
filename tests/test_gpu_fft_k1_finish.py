"""How a 64 x 64 patch ends under cv::phaseCorrelate's peak model (csrc/pc_kernel.hip): when one wave alone holds the surface's maximum,
that wave walks the index chain, reads its window element and stores the patch's 128-byte record while the other three leave; a maximum
attained in several waves (flat and periodic surfaces) goes through the second barrier to wave 0, which stores the same record.
pc_finish_kernel, one lane per patch, then adds the three fp64 sums in wave_sum3's pairing and runs peak_finish on the very operands the
tail had inside K1, so every result keeps its bits -- through every form, a batch that goes out in several pieces through the engine's
record buffer, and a captured graph. The fixture tests/golden/k1_finish.npz (made by tests/golden/make_k1_finish.py; the cases
and what each is for: tests/k1_finish_cases.py) was recorded ONCE on the GPU from the commit before that change; every float64 of the
shifts, through the default entry (quality null) and the _q entry, and of the quality must come out with the same bits."""
import os

import numpy as np
import pytest

import k1_finish_cases as K

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "k1_finish.npz")


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", [name for name, _ in K.CASES])
def test_same_bits_as_recorded(gpu, golden, name):
    got = dict(K.CASES)[name](golden, gpu)
    keys = sorted(k.split("/", 1)[1] for k in golden if k.startswith(name + "/"))
    assert keys == sorted(got) and keys == ["quality", "shift", "shift_q"], (keys, sorted(got))
    for key in keys:
        have, want = got[key], golden[f"{name}/{key}"]
        assert have.shape == want.shape, (name, key, have.shape, want.shape)
        bad = np.argwhere((_bits(have) != _bits(want)).any(axis=-1))
        for idx in bad[:8]:
            print(f"k1 finish [{name}] {key} {idx.tolist()}: got {have[tuple(idx)].tolist()} recorded {want[tuple(idx)].tolist()}")
        assert len(bad) == 0, (name, key, bad[:8].tolist(), len(bad))


def test_record_is_about_what_the_cases_name(golden):
    """the recorded results say that the inputs do what the cases claim (no GPU)"""
    # every wave ends a patch: wave w owns the un-shifted columns [8 w, 8 w + 8) and those + 32; the un-shifted peak column is the rounded
    # x shift mod 64 (the centroid lies within a pixel of the first maximum)
    s = golden["peak in each wave/shift"]
    assert not np.isnan(s).any()
    owners = sorted(((np.rint(s[:, 0, 0]).astype(int) % K.N % 32) // 8).tolist())
    assert owners == [0, 0, 1, 1, 2, 2, 3, 3], owners
    # the window is clamped: every pair has a component within two pixels of the edge of the shifted surface (+-32), or was gated for it
    sc = golden["clamped window/shift"][:, 0, :]
    assert not np.isnan(golden["clamped window/quality"]).any()
    assert ((np.abs(np.abs(np.nan_to_num(sc, nan=32.0)) - 31.0) <= 1.5).any(axis=1)).all(), sc.tolist()
    # the gate: pairs that pass max_px_speed = 4 and pairs that fail it, the quality stored either way
    sg = np.isnan(golden["gate/shift"][:, 0, 0])
    assert sg.any() and (~sg).any() and not np.isnan(golden["gate/quality"]).any(), sg.tolist()
    # flat surfaces: a constant patch answers 9 c / (9 c + eps) - 32 in both components, the all-zero pair (-32, -32)
    st = golden["several holders/shift"][:, 0]
    assert np.allclose(st[:3], -31.0, rtol=0, atol=1e-4) and (st[:3, 0] == st[:3, 1]).all() and st[3].tolist() == [-32.0, -32.0], st.tolist()
    # window offsets: none zero
    assert (np.abs(golden["pred"]).sum(axis=-1) > 0).all()


def test_second_piece_reuses_the_record_buffer(gpu):
    """65 540 pairs of one patch go out in two pieces (65 535 + 5), each the field kernel and then the finish kernel; the second piece
    writes its records from the start of the engine's buffer again and its shifts and quality at its own offsets. Pair k carries the bits
    recorded for pair k mod 8 of the first period (tests/golden/k1_prologue.npz, the batch tests/k1_prologue_cases.py builds)."""
    import k1_prologue_cases as KP
    from mrs_optic_flow_amd import FftMethod

    rec = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "k1_prologue.npz")))
    fm = FftMethod(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1))
    cur, prev = KP.split_batch(rec, gpu)
    assert cur.shape[0] == KP.SPLIT_PAIRS > 65535
    shifts, quality = fm.process_batch_device(cur, prev, return_quality=True)
    k = np.arange(KP.SPLIT_PAIRS) % KP.SPLIT_PERIOD
    for what, have, want in (("shift", shifts, rec["split period/shift_q"]), ("quality", quality, rec["split period/quality"])):
        off = np.argwhere((_bits(have.cpu().numpy()) != _bits(want)[k]).any(axis=(1, 2))).ravel()
        print(f"split, {what}: {len(k) - off.size} of {len(k)} pairs carry the recorded bits")
        assert off.size == 0, (what, off[:4].tolist(), int(off.size))
    # the same engine on a short batch afterwards: the buffer holds stale records of the long one behind the first eight
    again = fm.process_batch_device(cur[:8], prev[:8])
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(rec["split period/shift"]))


def test_captured_batch_replays_the_eager_bits(gpu, golden):
    """field kernel + finish kernel captured into one graph on a FRESH engine (the record buffer is made with the engine: nothing has to
    grow inside the capture), replayed twice on new inputs: the eager bits"""
    import torch

    from mrs_optic_flow_amd import FftMethod, release_captured

    cur, prev = (torch.from_numpy(golden[k]).to(gpu) for k in ("clamp_cur", "clamp_prev"))
    want_s, want_q = golden["clamped window/shift_q"], golden["clamped window/quality"]
    fm = FftMethod(sample_point_size=K.N, max_px_speed=1000.0, frame_shape=(K.N, K.N), grid=(1, 1))
    FftMethod(sample_point_size=K.N, frame_shape=(K.N, K.N), grid=(1, 1)).process_batch_device(cur, prev, return_quality=True)  # (another engine: the kernels are loaded)
    c, p = torch.zeros_like(cur), torch.zeros_like(prev)
    torch.cuda.synchronize()
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            s, q = fm.process_batch_device(c, p, return_quality=True)
    assert fm.graph_pinned
    c.copy_(cur)
    p.copy_(prev)
    for _ in range(2):
        s.zero_()
        q.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)) and np.array_equal(_bits(q.cpu().numpy()), _bits(want_q))
    del graph
    release_captured(fm)


def test_pieces_of_whole_frame_pairs_on_a_grid(gpu):
    """An 8 x 8 grid: the engine's buffer holds 65536 records, so a piece is 1024 frame pairs. 1030 pairs go out as 1024 + 6, the
    second piece at its own frame, shift and quality offsets with the records from the buffer's start again; 1024 pairs are exactly one
    piece. Pair k repeats pair k mod 8 of a batch of 8 (one piece, the same engine)."""
    import torch

    from mrs_optic_flow_amd import FftMethod

    rng = np.random.default_rng(7)
    scene = rng.integers(0, 256, (112, 112), dtype=np.uint8)  # nine crops of one scene, a few pixels apart
    protos = torch.from_numpy(np.stack([scene[5 + (j % 3):105 + (j % 3), 3 + (j % 4):103 + (j % 4)] for j in range(9)])).to(gpu)
    fm = FftMethod(sample_point_size=K.N, frame_shape=(100, 100), grid=(8, 8), stride=(5, 5))
    assert fm.kernel_variant == "stockham" and fm.n_patches == 64
    k = torch.arange(1030, device=gpu) % 8
    cur, prev = protos[k + 1], protos[k]
    want_s, want_q = (t.cpu().numpy() for t in fm.process_batch_device(cur[:8], prev[:8], return_quality=True))
    assert not np.isnan(want_q).any() and len({want_s[j].tobytes() for j in range(8)}) == 8  # (eight different pairs)
    kk = k.cpu().numpy()
    for n in (1030, 1024, 1025):
        s, q = fm.process_batch_device(cur[:n], prev[:n], return_quality=True)
        plain = fm.process_batch_device(cur[:n], prev[:n])
        for what, have, want in (("shift", s, want_s), ("quality", q, want_q), ("default entry", plain, want_s)):
            off = np.argwhere((_bits(have.cpu().numpy()) != _bits(want)[kk[:n]]).any(axis=(1, 2))).ravel()
            assert off.size == 0, (n, what, off[:4].tolist(), int(off.size))
