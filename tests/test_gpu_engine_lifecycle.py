"""GPU tests of the engines' lifetime (csrc/dev_mem.hpp: every device buffer, pinned buffer, stream and event of an engine is held by
an owner, teardown is `delete` after the waits). Each case reads mof_live_buffers() and mof_deferred_count(), creates ONE engine of the
smallest configuration that owns the resource in question, makes the calls that touch every lazily made resource (scratch regrowth,
the host pipes, BlockMethod::Refine's images), destroys the engine and asserts both counts are back where they started -- an exact
"nothing leaked", which free device memory cannot give on a GPU that other processes use. The results on the way are held to the
bits of the entry they must equal. Cases that need an environment knob (MOF_FFT_LARGE_PASS, MOF_HOST_CHUNK: read once per process)
and the parking case (mof_purge_deferred() frees EVERY parked engine of a process) run this module's functions in a child process."""
import contextlib
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _counts():
    from mrs_optic_flow_amd import _capi

    lib = _capi.load()
    return lib.mof_live_buffers(), lib.mof_deferred_count()


@contextlib.contextmanager
def _lifecycle(make):
    """make() -> engine; the body uses it; then it is closed and both counts must be back at their start."""
    gc.collect()  # (engines other tests dropped are finalised now, not in the middle of the case)
    start = _counts()
    engine = make()
    assert _counts()[0] > start[0] and _counts()[1] == start[1]
    try:
        yield engine
    finally:
        engine.close()
    assert _counts() == start, (_counts(), start)


def _frames(n, h, w, seed=5):
    from mrs_optic_flow_amd import synth

    canvas = synth.canvas_np(0, h + 3 * n + 8, w + 2 * n + 8, seed=seed)
    return np.stack([canvas[3 * k: 3 * k + h, 2 * k: 2 * k + w] for k in range(n)])


@pytest.mark.parametrize("patch,frame,variant", [(32, 64, None), (64, 128, None), (20, 40, "planned"), (60, 120, "planned-half")])
def test_fft_engine_in_lds(gpu, patch, frame, variant):
    """The tuned kernels at 32 and 64 (at 64 the fragment table lies behind the twiddles), the planned kernel (patch 20 on 40 x 40) and
    the half-tile default (patch 60 on 120 x 120): processImage twice."""
    from mrs_optic_flow_amd import FftMethod

    f = _frames(2, frame, frame)
    with _lifecycle(lambda: FftMethod(frame, patch, 80.0)) as fm:
        if variant:
            assert fm.kernel_variant == variant
        fm.processImage(f[0])
        out = fm.processImage(f[1])
        assert out.shape == (4, 2)


def large_pipeline_case():
    """Patch 200 on a 200 x 200 frame, grid 1 (the pipeline through HBM scratch, its fence): stateful calls, then a device batch of 3
    pairs -- the scratch grows from one pair to a pass -- whose shifts equal the stateful calls' bit for bit."""
    import torch

    from mrs_optic_flow_amd import FftMethod

    f = _frames(4, 200, 200)
    with _lifecycle(lambda: FftMethod(200, 200, 80.0)) as fm:
        assert fm.kernel_variant == "planned-large" and fm.n_patches == 1
        stateful = np.stack([fm.processImage(f[k]) for k in range(4)])[1:]  # (the first call correlates frame 0 with itself)
        live = _counts()[0]
        t = torch.from_numpy(f).cuda()
        got = fm.process_batch_device(t[1:], t[:-1]).cpu().numpy()
        assert _counts()[0] == live  # regrown in place: five buffers before, five after
        assert np.array_equal(got, stateful, equal_nan=True), (got, stateful)


def test_fft_large_pipeline(gpu):
    large_pipeline_case()


def test_fft_large_pipeline_across_a_pass_boundary(gpu):
    """MOF_FFT_LARGE_PASS=2: the 3 pairs take two passes of the scratch."""
    _child("large_pipeline_case", {"MOF_FFT_LARGE_PASS": "2"})


def test_block_matching_engine_with_refine(gpu):
    """16 / 8 / 8 on 96 x 160: processImage twice, then refine -- the two 2x images and the SAD buffers are made by its first call."""
    from mrs_optic_flow_amd import FastSpacedBMMethod

    f = _frames(2, 96, 160)
    with _lifecycle(lambda: FastSpacedBMMethod(16, 8, 8, (96, 160))) as bm:
        bm.processImage(f[0])
        mode = bm.processImage(f[1])[0]
        live = _counts()[0]
        x, y = bm.refine((int(mode[0]), int(mode[1])), 2)
        assert _counts()[0] == live + 4  # d_up[0], d_up[1], d_sad9, h_sad9
        assert np.isfinite([x, y]).all() and abs(x - mode[0]) <= 1 and abs(y - mode[1]) <= 1
        assert bm.refine((int(mode[0]), int(mode[1])), 2) == (x, y) and _counts()[0] == live + 4


@pytest.mark.parametrize("res,M", [(96, 24.0), (64, 18.0)])
def test_estimator_engine_with_scratch_regrowth(gpu, res, M):
    """The estimator on its tuned transforms (96) and on the planned pipeline (64): one stateful call, reserve(1), then a batch of 4
    pairs, so the scratch regrows; the live count is unchanged by the regrowth, and the batch equals what the stateful entry returns
    for a fresh estimator fed (prev, cur)."""
    import torch

    import sr_scenes
    from mrs_optic_flow_amd import ScaleRotationEstimator

    base = sr_scenes.canvas(3, res)
    v = np.stack([sr_scenes.view(base, res, 1.0 + 0.02 * k, 2.0 * k) for k in range(5)])
    with _lifecycle(lambda: ScaleRotationEstimator(res, M)) as est:
        assert est.processImage(v[0]) == (1.0, 0.0)
        est.reserve(1)
        live = _counts()[0]
        t = torch.from_numpy(v).cuda()
        got = est.process_batch_device(t[1:], t[:-1]).cpu().numpy()
        assert _counts()[0] == live
        assert np.isfinite(got).all() and not np.array_equal(got[0], got[3])
        for k in range(4):
            est.reset()
            est.processImage(v[k])
            assert est.processImage(v[k + 1]) == (got[k, 0], got[k, 1]), k


def host_pipes_case():
    """5 pairs through pipes of 2 pairs per chunk (MOF_HOST_CHUNK=2: three chunks, the last one ragged; a second call reuses the slots):
    FftMethod's host batch without and with quality (two pipes), the block matcher's, the estimator's host sequence at 96 -- each
    equal to the device entry's bits."""
    import torch

    import sr_scenes
    from mrs_optic_flow_amd import FastSpacedBMMethod, FftMethod, ScaleRotationEstimator

    f = _frames(6, 64, 64)
    f[3] = 200  # a constant frame: NaN results travel too
    t = torch.from_numpy(f).cuda()
    with _lifecycle(lambda: FftMethod(64, 32, 80.0)) as fm:
        want, want_q = (x.cpu().numpy() for x in fm.process_batch_device(t[1:], t[:-1], return_quality=True))
        live = _counts()[0]
        assert np.array_equal(fm.process_batch_host(f[1:].copy(), f[:-1].copy()), want, equal_nan=True)
        one_pipe = _counts()[0]
        assert one_pipe > live
        got, got_q = fm.process_batch_host(f[1:].copy(), f[:-1].copy(), return_quality=True)
        assert np.array_equal(got, want, equal_nan=True) and np.array_equal(got_q, want_q, equal_nan=True)
        two_pipes = _counts()[0]
        assert two_pipes > one_pipe
        assert np.array_equal(fm.process_batch_host(f[1:], f[:-1]), want, equal_nan=True)  # a video, the slots reused
        assert _counts()[0] == two_pipes
    f = _frames(6, 96, 160)
    t = torch.from_numpy(f).cuda()
    with _lifecycle(lambda: FastSpacedBMMethod(16, 8, 8, (96, 160))) as bm:
        want = [x.cpu().numpy() for x in bm.process_batch_device(t[1:], t[:-1])]
        for _ in range(2):
            got = bm.process_batch_host(f[1:].copy(), f[:-1].copy())
            assert all(np.array_equal(g, w) for g, w in zip(got, want))
    base = sr_scenes.canvas(3, 96)
    v = np.stack([sr_scenes.view(base, 96, 1.0 + 0.02 * k, 2.0 * k) for k in range(6)])
    with _lifecycle(lambda: ScaleRotationEstimator(96, 24.0)) as est:
        want = est.process_sequence_device(torch.from_numpy(v).cuda()).cpu().numpy()
        gated = est.last_gated
        est.reset()
        got = est.process_sequence_host(v)  # 6 frames, 4 per slot: 4 + 2
        assert np.array_equal(got, want) and est.last_gated == gated


def test_host_pipes(gpu):
    _child("host_pipes_case", {"MOF_HOST_CHUNK": "2"})


def parking_case():
    """A tuned-32 batch captured into a graph pins its engine: destroyed past Python's keep-alive set it is parked, not freed -- the
    live count stays up, one more engine is deferred, the graph replays to the eager bits; once the graph is gone mof_purge_deferred()
    frees it and both counts are back."""
    import torch

    from mrs_optic_flow_amd import FftMethod, _capi
    from mrs_optic_flow_amd import engine as E

    lib = _capi.load()
    f = _frames(4, 64, 64)
    t = torch.from_numpy(f).cuda()
    start = _counts()
    fm = FftMethod(64, 32, 80.0)
    want = fm.process_batch_device(t[1:], t[:-1]).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out = fm.process_batch_device(t[1:], t[:-1])
    live = _counts()[0]
    E._CAPTURED.discard(fm)
    del fm
    gc.collect()
    assert _counts() == (live, start[1] + 1) and live > start[0]
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    del g
    assert lib.mof_purge_deferred() == 1
    assert _counts() == start, (_counts(), start)


def test_parked_engine_keeps_its_buffers_until_purged(gpu):
    _child("parking_case", {})


def _child(case, env):
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {os.path.join(ROOT, 'tests')!r}]; import torch; import test_gpu_engine_lifecycle as T; T.{case}(); print('lifecycle ok')"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
    assert r.returncode == 0 and "lifecycle ok" in r.stdout, (case, env, r.stdout[-1500:], r.stderr[-2500:])
