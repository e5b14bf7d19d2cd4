"""GPU tests of the estimator's correlation quality and response gate (include/mof.h: mof_sr_*_q, mof_sr_set_min_response; K8 =
sr_final_kernel, L8 = pcl_final_kernel mode 0, sr_finish in csrc/pc_common.hpp).

Reference: tests/sr_quality_cases.py, the state machine around the unchanged oracle that test_sr_quality_host.py proves. Bar: both
slots of (response, peak) within 360 d of the f64 oracle, d = the distance of the f32 and the f64 oracle over the batch
(quality_cases.BAR_FACTOR, the rule of the FFT engine's quality tests); every measured maximum is printed next to its bar. Between the
entries of the library the bar is identity of bits: the same kernels run.

Which entries compute the same thing: the sequence entry and the stateful loop, on the whole video (frame 0 through INTER_CUBIC, every
later frame through INTER_LANCZOS4); the batch entry's pair k and a FRESH estimator fed (prev_k, cur_k) -- prev through INTER_CUBIC.
Pair 0 of the five views is all three."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sr_quality_cases as S
from mrs_optic_flow_amd import MofError, ScaleRotationEstimator, _capi, release_captured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_quality", "test_sr_quality")
PT_TOL, SR_TOL = 1e-4, 1e-5  # the project's bars on pt [px] and on (scale, rot)
IDENTITY = (1.0, 0.0)


def _hold(got_q, ref, what):
    """quality of the frames / pairs a correlation ran for against the f64 oracle, per slot"""
    ran = ~np.isnan(ref.quality[:, 0])
    assert np.isnan(got_q[~ran]).all(), (what, got_q[~ran])
    err = np.abs(got_q[ran] - ref.quality[ran]).max(axis=0)
    print(f"{what} [{ref.name}]: response off by {err[0]:.2e}, peak by {err[1]:.2e}; bar {ref.bar:.2e} (d = {ref.d:.2e})")
    assert (err <= ref.bar).all(), (what, err.tolist(), ref.bar)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _stateful(est, frames):
    """the processImage loop: [n, 2] (scale, rot), [n, 2] last_quality"""
    out, q = [], []
    for f in frames:
        out.append(est.processImage(f))
        q.append(est.last_quality.copy())
    return np.array(out), np.array(q)


def _parity(gpu, res, M, variant=0):
    v = S.views(res)
    tv = torch.tensor(v, device=gpu)
    new = lambda **kw: ScaleRotationEstimator(res, M, logpolar_variant=variant, **kw)  # noqa: E731
    ref_v, ref_p = S.route_video(res, M, variant), S.route_pairs(res, M, variant)
    # the batch entry
    est = new()
    out_b, q_b = est.process_batch_device(tv[1:], tv[:-1], return_quality=True)
    plain_b = est.process_batch_device(tv[1:], tv[:-1])
    assert torch.equal(out_b, plain_b)  # (scale, rot, pt): the same bits with and without the quality pointer
    out_b, q_b = out_b.cpu().numpy(), q_b.cpu().numpy()
    _hold(q_b, ref_p, f"{res} batch")
    assert np.abs(out_b[:, 2:] - ref_p.out[:, 2:]).max() <= PT_TOL
    for k in range(len(v) - 1):  # ... is the two-call sequence of a fresh estimator
        one = new()
        assert one.processImage(v[k]) == IDENTITY and np.isnan(one.last_quality).all()
        assert one.processImage(v[k + 1]) == (out_b[k, 0], out_b[k, 1]), (res, k)
        assert np.array_equal(one.last_quality, q_b[k]), (res, k, one.last_quality, q_b[k])
    # the sequence entry, resolved and asynchronous, with and without quality
    out_s, q_s = new().process_sequence_device(tv, return_quality=True)
    assert torch.equal(out_s, new().process_sequence_device(tv))
    out_a, q_a = new().process_sequence_device(tv, resolve_gate=False, return_quality=True)
    assert torch.equal(out_a, new().process_sequence_device(tv, resolve_gate=False))
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_s) and _same(q_a.cpu().numpy(), q_s.cpu().numpy())  # (nothing is gated)
    out_s, q_s = out_s.cpu().numpy(), q_s.cpu().numpy()
    assert np.isnan(q_s[0]).all() and tuple(out_s[0]) == (1.0, 0.0, 0.0, 0.0)  # no correlation ran
    _hold(q_s, ref_v, f"{res} sequence")
    assert np.abs(out_s[1:, 2:] - ref_v.out[1:, 2:]).max() <= PT_TOL
    # the stateful loop
    out_1, q_1 = _stateful(new(), v)
    assert np.array_equal(out_1, out_s[:, :2]) and _same(q_1, q_s), (res, q_1, q_s)
    assert np.array_equal(q_s[1], q_b[0])  # frame 1 of the video is pair 0 of the batch


@pytest.mark.parametrize("res,M", S.ROUTES)
def test_parity_per_route(gpu, res, M):
    """The five views of test_scale_rotation_at_any_resolution at the smallest resolution of every route (sr_quality_cases.ROUTE_NOTES):
    batch entry, stateful loop and sequence entry; quality within the bar, identical bits between the entries, (NaN, NaN) for frame 0 of
    a fresh estimator, (scale, rot, pt) untouched by the quality pointer."""
    _parity(gpu, res, M)


def test_parity_with_the_opencv3_map(gpu):
    from mrs_optic_flow_amd.engine import LOGPOLAR_CV3
    _parity(gpu, 100, 22.0, LOGPOLAR_CV3)


def test_parity_on_the_planned_pipeline_everywhere(gpu):
    """MOF_SR_TUNED_ALL=0 (read once per process: a fresh child): 100 runs L5 - L8, 240 stays on the tuned transforms"""
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-m", "gpu", "-k",
                          "test_parity_per_route and (100 or 240)", "-p", "no:cacheprovider"],
                         env=dict(os.environ, MOF_SR_TUNED_ALL="0"), capture_output=True, text=True, timeout=600, cwd=ROOT)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "2 passed" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


def test_passes_and_pitch(gpu):
    """Nine frames through passes of four (frame 0, then 4 + 4), inside a wider buffer (pitch > res, the crop origin passed as the
    pointer): results and quality of the whole-video call on the dense video, bit for bit"""
    res, M = 100, 22.0
    frames = S.views(res)[[0, 1, 2, 3, 4, 2, 0, 3, 1]]
    dense = torch.tensor(frames, device=gpu)
    wide = torch.zeros((len(frames), res + 2, res + 24), dtype=torch.uint8, device=gpu)
    wide[:, 1:1 + res, 8:8 + res] = dense
    want, want_q = ScaleRotationEstimator(res, M).process_sequence_device(dense, return_quality=True)
    for resolve in (True, False):
        got, got_q = ScaleRotationEstimator(res, M, batch_chunk=4).process_sequence_device(wide[:, 1:1 + res, 8:8 + res], resolve_gate=resolve,
                                                                                           return_quality=True)
        torch.cuda.synchronize()
        assert torch.equal(got, want) and _same(got_q.cpu().numpy(), want_q.cpu().numpy()), resolve
    assert torch.isfinite(want_q[1:]).all()


def test_reference_gate_with_quality(gpu):
    """The 600 noise frames of test_sequence_gate_leaves_prev_unchanged: the resolved call's quality is the stateful loop's
    last_quality on every frame -- the frame behind the first gated one included, whose pair was re-run against an older partner and
    whose quality therefore differs from the unresolved run's -- and a gated frame reports the (finite) quality of what gated it."""
    res, M, n = 240, 40.0, 600
    frames = np.random.default_rng(2024).integers(0, 256, (n, res, res), dtype=np.uint8)
    video = torch.tensor(frames, device=gpu)
    raw, raw_q = ScaleRotationEstimator(res, M, batch_chunk=128).process_sequence_device(video, resolve_gate=False, return_quality=True)
    est = ScaleRotationEstimator(res, M, batch_chunk=128)
    got, got_q = est.process_sequence_device(video, return_quality=True)
    torch.cuda.synchronize()
    raw, raw_q, got, got_q = (t.cpu().numpy() for t in (raw, raw_q, got, got_q))
    want, want_q = _stateful(ScaleRotationEstimator(res, M), frames)
    assert np.array_equal(got[:, :2], want) and _same(got_q, want_q)
    gated = np.flatnonzero(np.abs(got[:, 2]) > res / 2)
    assert est.last_gated == gated.size and gated.size >= 1
    print(f"{gated.size} gated frames of {n}, the first at {int(gated[0])}; their responses {got_q[gated, 0].min():.3f} .. {got_q[gated, 0].max():.3f}")
    assert np.isfinite(got_q[gated]).all() and np.isnan(got_q[0]).all() and np.isfinite(got_q[1:]).all()
    g0 = int(gated[0])
    assert g0 + 1 < n and np.array_equal(got_q[:g0 + 1], raw_q[:g0 + 1], equal_nan=True)
    assert not np.array_equal(got_q[g0 + 1], raw_q[g0 + 1])


@pytest.mark.parametrize("res,M", S.GATE_CASES)
def test_response_gate(gpu, res, M):
    """[v0, v1, v2, noise, v3, v4] under min_response = 0.4 (test_sr_quality_host.py: matched responses >= 0.6, noise pairs <= 0.27 on
    both oracles, pt.x of the noise pairs inside the reference's gate): every entry gates what the helper's state machine gates."""
    refs, f = S.gate_refs(res, M), S.gate_video(res)
    tf = torch.tensor(f, device=gpu)
    ref = refs["video"]
    new = lambda mr=S.MIN_RESPONSE, **kw: ScaleRotationEstimator(res, M, min_response=mr, **kw)  # noqa: E731
    one = new()
    assert one.min_response == S.MIN_RESPONSE
    out_1, q_1 = _stateful(one, f)
    _hold(q_1, ref, f"{res} gated, stateful")
    keep = ~ref.gated
    assert ref.gated.tolist() == [k == S.NOISE_AT for k in range(len(f))]
    assert tuple(out_1[S.NOISE_AT]) == IDENTITY
    assert np.abs(out_1[keep] - ref.out[keep, :2]).max() < SR_TOL
    for chunk in (0, 2):  # the resolved sequence entry; passes of two put the gated frame and the one behind it into different passes
        est = new(batch_chunk=chunk)
        got, got_q = est.process_sequence_device(tf, return_quality=True)
        assert est.last_gated == 1
        plain = new(batch_chunk=chunk)
        assert torch.equal(plain.process_sequence_device(tf), got) and plain.last_gated == 1  # (the walk reads the engine's own scratch)
        got, got_q = got.cpu().numpy(), got_q.cpu().numpy()
        assert np.array_equal(got[:, :2], out_1) and _same(got_q, q_1), chunk
        assert np.abs(got[1:, 2:] - ref.out[1:, 2:]).max() <= PT_TOL  # pt is still reported for frame 3; frame 4 is the (v3, v2) pair
        # the state after the video: the next stateful call agrees between the engines and with the helper
        nxt = S.views(res)[1]
        step = copy.copy(ref.machine).step(nxt)
        a, b = one.processImage(nxt) if chunk == 0 else None, est.processImage(nxt)
        assert (a is None or a == b) and abs(b[0] - step[0][0]) < SR_TOL and abs(b[1] - step[0][1]) < SR_TOL and not step[3]
        assert np.abs(est.last_quality - step[1]).max() <= S.BAR_FACTOR * max(ref.d, np.abs(step[2] - step[1]).max())  # (d of the video and this frame)
    # the asynchronous form: the output is gated, every frame has its immediate predecessor -- frame 4 meets the noise frame
    ref_a = refs["consecutive"]
    est = new()
    got, got_q = est.process_sequence_device(tf, resolve_gate=False, return_quality=True)
    torch.cuda.synchronize()
    got, got_q = got.cpu().numpy(), got_q.cpu().numpy()
    _hold(got_q, ref_a, f"{res} gated, asynchronous")
    assert ref_a.gated.tolist() == [k in (S.NOISE_AT, S.NOISE_AT + 1) for k in range(len(f))]
    assert all(tuple(got[k, :2]) == IDENTITY for k in (S.NOISE_AT, S.NOISE_AT + 1))
    assert np.abs(got[~ref_a.gated, :2] - ref_a.out[~ref_a.gated, :2]).max() < SR_TOL
    assert np.abs(got[1:, 2:] - ref_a.out[1:, 2:]).max() <= PT_TOL
    # the batch entry: pairs are independent, exactly the two that hold the noise frame change -- and only in (scale, rot)
    ref_p = refs["pairs"]
    on, on_q = new().process_batch_device(tf[1:], tf[:-1], return_quality=True)
    off, off_q = new(0.0).process_batch_device(tf[1:], tf[:-1], return_quality=True)
    on, on_q, off, off_q = (t.cpu().numpy() for t in (on, on_q, off, off_q))
    _hold(on_q, ref_p, f"{res} gated, batch")
    assert np.array_equal(on_q, off_q) and np.array_equal(on[:, 2:], off[:, 2:])  # the value does not depend on the gate
    for k in range(len(f) - 1):
        if ref_p.gated[k]:
            assert k in (S.NOISE_AT - 1, S.NOISE_AT) and tuple(on[k, :2]) == IDENTITY and tuple(off[k, :2]) != IDENTITY, k
        else:
            assert np.array_equal(on[k], off[k]), k
    # min_response = 0: frame 3 is not gated, becomes the previous image, and the bits do not depend on how the engine got to 0
    ref_0 = refs["off"]
    dflt = ScaleRotationEstimator(res, M)
    got0, q0 = dflt.process_sequence_device(tf, return_quality=True)
    assert dflt.last_gated == 0 and dflt.min_response == 0.0
    back = new()
    back.set_min_response(0.0)
    assert torch.equal(back.process_sequence_device(tf), got0)
    got0, q0 = got0.cpu().numpy(), q0.cpu().numpy()
    _hold(q0, ref_0, f"{res} gate off")
    assert tuple(got0[S.NOISE_AT, :2]) != IDENTITY and np.abs(got0[:, :2] - ref_0.out[:, :2]).max() < SR_TOL
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(MofError) as exc:
            dflt.set_min_response(bad)
        assert exc.value.code == _capi.MOF_ERR_BAD_ARG


def test_zero_frames(gpu):
    """An all-zero frame has an all-zero log-polar image and the surface is flat zero: quality exactly (0, 0), on either side of the
    pair, and pt what the entry without quality returns"""
    res, M = 100, 22.0
    v, z = S.views(res)[1], np.zeros((res, res), np.uint8)
    cur, prev = torch.tensor(np.stack([z, v]), device=gpu), torch.tensor(np.stack([v, z]), device=gpu)
    est = ScaleRotationEstimator(res, M)
    out, q = est.process_batch_device(cur, prev, return_quality=True)
    assert torch.equal(out, est.process_batch_device(cur, prev))
    assert (q.cpu().numpy() == 0.0).all(), q
    for a, b in ((z, v), (v, z)):
        one = ScaleRotationEstimator(res, M)
        one.processImage(a)
        one.processImage(b)
        assert (one.last_quality == 0.0).all(), one.last_quality
    # under the response gate a flat zero surface is gated: 0 >= min_response is false
    on = ScaleRotationEstimator(res, M, min_response=S.MIN_RESPONSE).process_batch_device(cur, prev).cpu().numpy()
    assert all(tuple(on[k, :2]) == IDENTITY for k in range(2)) and np.array_equal(on[:, 2:], out.cpu().numpy()[:, 2:])


def test_graph_capture_and_the_pinned_setter(gpu):
    """A _q batch captured on an armed, reserved engine replays with the plain call's bits; the gate value is an argument of the captured
    kernel, so the setter refuses a pinned engine and works again once its graphs are released"""
    res, M = 100, 22.0
    v = torch.tensor(S.views(res), device=gpu)
    est = ScaleRotationEstimator(res, M, min_response=S.MIN_RESPONSE)
    est.processImage(S.views(res)[0])
    est.reserve(4)
    want, want_q = (t.clone() for t in est.process_batch_device(v[1:], v[:-1], return_quality=True))
    assert torch.equal(want, est.process_batch_device(v[1:], v[:-1]))
    torch.cuda.synchronize()
    g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            out, q = est.process_batch_device(v[1:], v[:-1], return_quality=True)
    for _ in range(2):
        out.zero_()
        q.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want) and torch.equal(q, want_q)
    assert est.graph_pinned
    with pytest.raises(MofError) as exc:
        est.set_min_response(0.3)
    assert exc.value.code == _capi.MOF_ERR_BUSY and est.min_response == S.MIN_RESPONSE
    del exc, g
    assert release_captured(est) == 1 and not est.graph_pinned
    est.set_min_response(0.3)
    assert est.min_response == 0.3


def test_host_entry_and_cpp_mirror(gpu, tmp_path, monkeypatch):
    """process_sequence_host(return_quality=True) over three upload chunks of two frames is the device entry, bit for bit, and the C++
    mirror's lastQuality(), processSequenceDeviceQ and processVideoQ print the Python binding's values -- on the gate video, gate armed"""
    assert os.path.exists(BIN), "tests/cpp_quality/test_sr_quality missing: run __graft_entry__.build()"
    res, M = 100, 22.0
    f = S.gate_video(res)
    want, want_q = ScaleRotationEstimator(res, M, min_response=S.MIN_RESPONSE).process_sequence_device(torch.tensor(f, device=gpu), return_quality=True)
    want, want_q = want.cpu().numpy(), want_q.cpu().numpy()
    out_1, q_1 = _stateful(ScaleRotationEstimator(res, M, min_response=S.MIN_RESPONSE), f)
    monkeypatch.setenv("MOF_HOST_CHUNK", "1")  # (read when an engine's host pipeline is made: a slot of the frames form holds two chunks)
    for mr in (S.MIN_RESPONSE, 0.0):
        est = ScaleRotationEstimator(res, M, min_response=mr)
        got, got_q = est.process_sequence_host(f, return_quality=True)
        dev = ScaleRotationEstimator(res, M, min_response=mr)
        d, d_q = dev.process_sequence_device(torch.tensor(f, device=gpu), return_quality=True)
        assert np.array_equal(got, d.cpu().numpy()) and _same(got_q, d_q.cpu().numpy()) and est.last_gated == dev.last_gated == (1 if mr else 0)
        plain = ScaleRotationEstimator(res, M, min_response=mr)
        assert np.array_equal(plain.process_sequence_host(f), got) and plain.last_gated == est.last_gated
    path = tmp_path / "video.u8"
    f.tofile(path)
    r = subprocess.run([BIN, str(res), repr(M), repr(S.MIN_RESPONSE), str(len(f)), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = r.stdout.split("\n")
    assert lines[0].split() == ["gated", "1", "1"], lines[0]
    for t in range(len(f)):
        w = lines[1 + t].split()
        assert w[:3] == ["frame", str(t), "stateful"] and w[7] == "device" and w[14] == "host", w
        one, dev, host = (np.array([float(x) for x in w[a:b]]) for a, b in ((3, 7), (8, 14), (15, 21)))
        assert _same(one, np.concatenate([out_1[t], q_1[t]])), (t, one)
        assert _same(dev, np.concatenate([want[t], want_q[t]])) and _same(host, dev), (t, dev, host)
