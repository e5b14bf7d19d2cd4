"""GPU tests of the FFT engine's opt-in response gate (include/mof.h, mof_fft_set_min_response; csrc/pc_gate_kernel.hip).

Reference for the bits: the SAME engine unarmed -- its shifts and quality are held to the CPU oracle by test_gpu_fft_quality.py and the
shift tests. Inputs, thresholds and expected gated sets: tests/gate_cases.py, whose classes test_fft_gate_host.py shows to lie at least
1000 quality bars apart in both oracles; the threshold v of a batch is the midpoint of the f64 oracle's gap, nothing is taken from a GPU.
Every test asserts, through _gate_properties:
  - the armed quality has the unarmed quality's bits;
  - the armed shifts are, bit for bit, where(!(q0 >= v), NaN, unarmed shifts), q0 the unarmed stored response;
  - the gated set is the oracle's, and a patch the reference's validity rule already made NaN stays NaN;
  - the call without return_quality (the engine's own quality buffer) gives the same shift bits;
  - set_min_response(0) restores the unarmed bits."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gate_cases as GC
import quality_cases as Q
from mrs_optic_flow_amd import FftMethod, MofError, _capi, geometry as G, release_captured
from mrs_optic_flow_amd.engine import PEAK_OCL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_gate", "test_fft_gate")


def _np(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _bits(a):
    return np.ascontiguousarray(_np(a)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _engine(g, **kw):
    h, w = g.cur.shape[1:3]
    if g.ocl:
        kw.setdefault("peak_model", PEAK_OCL)
    return FftMethod(sample_point_size=g.n, max_px_speed=Q.SPEED, frame_shape=(h, w), grid=g.grid, **kw)


def _expected(s0, q0, v):
    """where(!(q0 >= v), NaN, s0)"""
    want = _np(s0).copy()
    want[~(_np(q0)[..., 0] >= v)] = np.nan
    return want


def _gate_properties(fm, run, v, gated, what, invalid=None):
    """run(return_quality) -> (shifts, quality) | shifts on engine fm, which arrives unarmed. gated [pairs, patches]: the oracle's set;
    invalid: the patches the validity rule makes NaN in the oracle (default: none may be). Leaves fm unarmed; returns the unarmed and
    the armed (shifts, quality) as numpy arrays."""
    assert fm.min_response == 0.0
    s0, q0 = (_np(t) for t in run(True))
    fm.set_min_response(v)
    assert fm.min_response == v
    s1, q1 = (_np(t) for t in run(True))
    plain = _np(run(False))
    fm.set_min_response(0.0)
    s2, q2 = (_np(t) for t in run(True))
    torch.cuda.synchronize()
    nan0, nan1 = np.isnan(s0[..., 0]), np.isnan(s1[..., 0])
    print(f"{what}: v = {v:.6f} gates {int((nan1 & ~nan0).sum())} of {nan1.size} patches ({int(nan0.sum())} invalid before the gate)")
    assert _same_bits(q1, q0), (what, "the stored quality must not depend on the gate")
    assert _same_bits(s1, _expected(s0, q0, v)), (what, np.argwhere(_bits(s1) != _bits(_expected(s0, q0, v))).tolist()[:8])
    assert np.array_equal(~(q0[..., 0] >= v), gated), (what, np.argwhere(~(q0[..., 0] >= v) != gated).tolist()[:8])
    assert np.array_equal(nan0, np.zeros_like(gated) if invalid is None else invalid), (what, np.argwhere(nan0).tolist()[:8])
    assert np.array_equal(nan1, gated | nan0) and np.array_equal(np.isnan(s1[..., 1]), nan1), what
    assert _same_bits(plain, s1), (what, "the call without a quality buffer must gate the same patches")
    assert _same_bits(s2, s0) and _same_bits(q2, q0), (what, "set_min_response(0) must restore the unarmed engine")
    return s0, q0, s1, q1


def _pair_runner(fm, cur, prev, gpu):
    c, p = torch.tensor(cur, device=gpu), torch.tensor(prev, device=gpu)  # (a copy: the batches' arrays are read-only)
    return lambda rq: fm.process_batch_device(c, p, return_quality=rq)


# ---- 1. per family, pair entry ----
@pytest.mark.parametrize("n,variant", GC.FAMILY_SIZES)
def test_per_family(gpu, n, variant):
    """Six single-patch pairs, odd ones unrelated: K1 (32, 64), the half tile (120, 142 -> 144), the planned kernel (54, 62 -> 64), the large
    pipeline (200, 196 -> 200)"""
    g = GC.family(n)
    fm = _engine(g)
    assert fm.kernel_variant == variant, fm.kernel_variant
    _gate_properties(fm, _pair_runner(fm, g.cur, g.prev, gpu), g.v, g.gated, f"n={n} {variant}", g.invalid)


# ---- 2. gate kernel indexing ----
def test_gate_kernel_indexing_320_patches(gpu):
    """320 patches: one full workgroup of the gate kernel and a ragged one; exactly the flat indices 0, 255, 256, 319 are gated"""
    g = GC.index320()
    fm = _engine(g)
    _, _, s1, _ = _gate_properties(fm, _pair_runner(fm, g.cur, g.prev, gpu), g.v, g.gated, "8 x 8 x 5 patches of 32", g.invalid)
    assert np.flatnonzero(np.isnan(s1[..., 0]).ravel()).tolist() == [0, 255, 256, 319]


def test_gate_kernel_indexing_3x2_grid(gpu):
    """7 pairs of a 3 x 2 grid, the unrelated patch of pair k at patch k mod 6: a transposed patch index gates another one"""
    g = GC.grid7()
    fm = _engine(g)
    _, _, s1, _ = _gate_properties(fm, _pair_runner(fm, g.cur, g.prev, gpu), g.v, g.gated, "3 x 2 x 7 patches of 64", g.invalid)
    assert [np.flatnonzero(r).tolist() for r in np.isnan(s1[..., 0])] == [[k % 6] for k in range(7)]


# ---- 3. the threshold's edge ----
def test_threshold_edge(gpu):
    """v = one matched patch's stored response, bit for bit: the patch passes (the gate is !(response >= v)); v = the next double: only
    that patch changes"""
    g = GC.grid7()
    fm = _engine(g)
    run = _pair_runner(fm, g.cur, g.prev, gpu)
    s0, q0 = (_np(t) for t in run(True))
    r = q0[..., 0]
    k, p = np.unravel_index(np.argmin(np.where(g.unrelated, np.inf, r)), r.shape)  # the weakest matched patch: nothing matched lies below it
    v = float(r[k, p])
    fm.set_min_response(v)
    at, at_plain = _np(run(True)[0]), _np(run(False))
    fm.set_min_response(float(np.nextafter(v, np.inf)))
    above = _np(run(True)[0])
    assert _same_bits(at, _expected(s0, q0, v)) and _same_bits(at_plain, at) and _same_bits(at[k, p], s0[k, p]) and np.isfinite(at[k, p]).all()
    differs = (_bits(at) != _bits(above)).any(axis=-1)
    assert np.argwhere(differs).tolist() == [[k, p]] and np.isnan(above[k, p]).all(), np.argwhere(differs).tolist()


# ---- 4. a constant patch ----
def test_constant_patch_n64(gpu):
    """A 64 x 64 texture against a constant patch under cv::phaseCorrelate's model: unarmed a finite, "valid" shift of (-31, -31); armed at
    the batch's v it is NaN and its quality keeps its bits"""
    g = GC.family(64)
    tex = np.random.default_rng(11).integers(0, 256, (1, 64, 64), dtype=np.uint8)
    cur, prev = np.concatenate([g.cur, tex]), np.concatenate([g.prev, np.full((1, 64, 64), 81, np.uint8)])
    gated = np.concatenate([g.gated, [[True]]])
    fm = _engine(g)
    s0, q0, s1, q1 = _gate_properties(fm, _pair_runner(fm, cur, prev, gpu), g.v, gated, "n=64 with a constant patch")
    print(f"constant patch: unarmed shift {s0[6, 0].tolist()}, response {q0[6, 0, 0]:.3e}")
    # (the f64 oracle's shift is -31 - 4.2e-6, test_fft_gate_host.py prints it; the project's shift bar is 1e-4 px: 2e-4 around -31)
    assert np.abs(s0[6, 0] + 31.0).max() < 2e-4 and 0.0 <= q0[6, 0, 0] < 1e-6
    assert np.isnan(s1[6, 0]).all() and _same_bits(q1[6], q0[6])


# ---- 5. the OpenCL kernel's model ----
@pytest.mark.parametrize("n,variant", GC.OCL_SIZES)
def test_opencl_model(gpu, n, variant):
    """MOF_PEAK_OCL on its own scale (refine()'s sum); a constant patch has a NaN response there: NaN unarmed, and gated when armed"""
    g = GC.ocl(n)
    tex = np.random.default_rng(11).integers(0, 256, (1, n, n), dtype=np.uint8)
    cur, prev = np.concatenate([g.cur, tex]), np.concatenate([g.prev, np.full((1, n, n), 81, np.uint8)])
    fm = _engine(g)
    assert fm.kernel_variant == variant, fm.kernel_variant
    s0, q0, s1, q1 = _gate_properties(fm, _pair_runner(fm, cur, prev, gpu), g.v, np.concatenate([g.gated, [[True]]]),
                                      f"OpenCL model n={n} {variant}", np.concatenate([g.invalid, [[True]]]))
    assert np.isnan(q0[6]).all() and np.isnan(s1[6]).all()


# ---- 6. videos ----
@pytest.mark.parametrize("n", GC.VIDEO_SIZES)
def test_videos(gpu, n):
    """process_sequence_device on five frames of two patches, frame 2 unrelated: K1s (64), the half tile's video form (120), the 128
    half-tile sequence kernel, the large video form (200). Pairs 1 and 2 are gated; pairs 0 and 3 keep their bits -- the spectrum a
    workgroup carries from frame to frame is not disturbed by the gate"""
    g = GC.video(n)
    fm = _engine(g)
    f = torch.tensor(g.frames, device=gpu)
    s0, _, s1, _ = _gate_properties(fm, lambda rq: fm.process_sequence_device(f, return_quality=rq), g.v, g.gated, f"video n={n} ({fm.kernel_variant})",
                                    g.invalid)
    assert np.isnan(s1[1:3]).all() and _same_bits(s1[[0, 3]], s0[[0, 3]]) and np.isfinite(s1[[0, 3]]).all()


def test_bgr8_entries_n64(gpu):
    """the BGR8 pair and video entries on the tinted frames of the 64-pixel video"""
    g = GC.bgr64()
    fm = _engine(g)
    f = torch.tensor(g.bgr, device=gpu)
    _gate_properties(fm, lambda rq: fm.process_sequence_device_bgr(f, return_quality=rq), g.v, g.gated, "BGR8 video n=64", g.invalid)
    _gate_properties(fm, lambda rq: fm.process_batch_device_bgr(f[1:], f[:-1], return_quality=rq), g.v, g.gated, "BGR8 pairs n=64", g.invalid)


# ---- 7. the long-range mode ----
def test_long_range(gpu):
    """128 / 32, four pairs, pairs 1 and 3 unrelated: the batch entry; processImageLongRange counts the gated patch in last_invalid and
    hands out its quality intact"""
    g = GC.long_range()
    fm = FftMethod(128, 32, Q.SPEED)
    c, p = torch.tensor(g.cur, device=gpu), torch.tensor(g.prev, device=gpu)
    s0, q0, s1, _ = _gate_properties(fm, lambda rq: fm.process_long_range_batch_device(c, p, return_quality=rq), g.v, g.gated, "long range 128 / 32",
                                     g.invalid)
    fm.set_min_response(g.v)
    for k in range(4):
        fm.processImageLongRange(g.prev[k])
        s = fm.processImageLongRange(g.cur[k])
        assert _same_bits(s, s1[k]) and _same_bits(fm.last_quality, q0[k]) and fm.last_invalid == int(g.gated[k].sum()), k


# ---- 8. the stateful entry ----
def test_stateful_process_image(gpu):
    """processImage on (prev k, cur k, prev k + 1) of the 3 x 2 grid, an armed engine beside an unarmed one: the armed engine's second call gates
    a patch and counts it; its third call has the unarmed engine's quality bits and its shifts under the gate -- the gated frame became
    the previous one (FftMethod.cpp:1872)"""
    g = GC.grid7()
    k = next(k for k in range(7) if not g.invalid[k].any())  # (a pair whose unrelated patch the validity rule lets through, by the oracle)
    armed, plain = _engine(g, min_response=g.v), _engine(g)
    assert armed.min_response == g.v
    for fm in (armed, plain):
        fm.processImage(g.prev[k])
    s1, s0 = armed.processImage(g.cur[k]), plain.processImage(g.cur[k])
    assert _same_bits(armed.last_quality, plain.last_quality) and _same_bits(s1, _expected(s0, plain.last_quality, g.v))
    assert np.flatnonzero(np.isnan(s1[:, 0])).tolist() == [k % 6] and armed.last_invalid == 1 and plain.last_invalid == 0
    nxt = g.prev[(k + 1) % 7]
    t1, t0 = armed.processImage(nxt), plain.processImage(nxt)
    assert _same_bits(armed.last_quality, plain.last_quality) and _same_bits(t1, _expected(t0, plain.last_quality, g.v))
    assert np.isfinite(plain.last_quality).all() and armed.last_invalid == int(np.isnan(t1[:, 0]).sum())
    armed.reset()
    assert armed.min_response == g.v, "mof_fft_reset keeps the value"


# ---- 9. the host entry ----
def test_host_entry(gpu):
    """process_batch_host on the 7 pairs of the 3 x 2 grid (in one chunk by default; in four chunks of two with a ragged last one under
    MOF_HOST_CHUNK=2, in the child of test_forced_passes_and_chunks): the device entry's armed bits"""
    g = GC.grid7()
    fm = _engine(g)
    _, _, s1, _ = _gate_properties(fm, lambda rq: fm.process_batch_host(g.cur, g.prev, return_quality=rq), g.v, g.gated, "host entry, 3 x 2 x 7", g.invalid)
    fm.set_min_response(g.v)
    assert _same_bits(_pair_runner(fm, g.cur, g.prev, gpu)(False), s1)


# ---- 10. the forms a knob selects, in child processes ----
def _env_cases(default):
    v = os.environ.get("MOF_GATE_CASES")
    return default if v is None else [tuple(item.split("=")) for item in v.split(",") if item]


@pytest.mark.parametrize("name,variant", _env_cases([("passes-200", "planned-large")]))
def test_pair_entry_on_its_route(gpu, name, variant):
    """A registered batch through the pair entry of the route this process takes. By default the 10 pairs of two 200-pixel patches in one
    pass; the children below select it with MOF_GATE_CASES under the knob they set."""
    g = GC.BATCHES[name]()
    fm = _engine(g)
    print(f"route {name}: kernel_variant {fm.kernel_variant}")
    assert fm.kernel_variant == variant, (name, fm.kernel_variant)
    _gate_properties(fm, _pair_runner(fm, g.cur, g.prev, gpu), g.v, g.gated, f"{g.name} ({fm.kernel_variant})", g.invalid)


_DIED = []  # a child that ended on a signal or at its time limit: no later test starts another on the same card


def _child(env, select, cases, passed):
    if _DIED:
        pytest.fail(f"not started: an earlier child of this module died ({_DIED[0]}); find its cause first")
    e = dict(os.environ, **env, MOF_GATE_CASES=",".join(f"{n}={v}" for n, v in cases))
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k", select, "-p", "no:cacheprovider"],
                           capture_output=True, text=True, timeout=300, cwd=ROOT, env=e)
    except subprocess.TimeoutExpired:
        _DIED.append(f"{env}: no end within 300 s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DIED.append(f"{env}: status {r.returncode}")
    for line in r.stdout.splitlines():
        if "gates " in line or "route " in line or " passed" in line:
            print(f"[{' '.join(f'{k}={v}' for k, v in env.items())}] {line}")
    assert r.returncode == 0 and f"{passed} passed" in r.stdout and " skipped" not in r.stdout, (env, r.returncode, r.stdout[-3000:], r.stderr[-1500:])
    for name, variant in cases:
        assert f"route {name}: kernel_variant {variant}" in r.stdout, (env, name, variant, r.stdout[-3000:])


def test_forced_passes_and_chunks(gpu):
    """MOF_FFT_LARGE_PASS=3, MOF_HOST_CHUNK=2 (read once per process): the 10 pairs at 200 take four passes of the large pipeline's scratch
    and ONE gate launch over all of them; the host entry's 7 pairs go up in four chunks, each with a gate launch of its own"""
    _child({"MOF_FFT_LARGE_PASS": "3", "MOF_HOST_CHUNK": "2"}, "test_pair_entry_on_its_route or test_host_entry", [("passes-200", "planned-large")], 2)


def test_the_older_forms(gpu):
    """MOF_PLANNED_STATIC=0, MOF_FFT_HALF=0 (they act on different sizes): 54 on the run-time plan of the planned kernel, 120 on the tuned
    kernel of pc_kernel_mixed.hip instead of the half tile (kernel_variant 'stockham' there; nothing exposes MOF_PLANNED_STATIC)"""
    _child({"MOF_PLANNED_STATIC": "0", "MOF_FFT_HALF": "0"}, "test_pair_entry_on_its_route", [("family-54", "planned"), ("family-120", "stockham")], 2)


# ---- 11. graphs ----
def test_graph_capture_and_replay(gpu):
    """An armed batch without a quality buffer: a capture on a fresh engine would have to grow the engine's quality buffer and is refused
    before anything is launched (MOF_ERR_BAD_ARG, the engine stays unpinned); after one eager run the same capture succeeds, replays the
    eager bits, pins the engine, and the setter answers MOF_ERR_BUSY until release_captured"""
    g = GC.grid7()
    fm = _engine(g, min_response=g.v)
    c, p = torch.tensor(g.cur, device=gpu), torch.tensor(g.prev, device=gpu)
    out, marker = torch.full((7, 6, 2), 7.0, dtype=torch.float64, device=gpu), torch.zeros(1, device=gpu)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(refused, stream=side):
            marker.add_(1.0)  # (so that the refused call leaves no empty graph behind)
            with pytest.raises(MofError) as exc:
                fm.process_batch_device(c, p, out=out)
    torch.cuda.synchronize()
    assert exc.value.code == _capi.MOF_ERR_BAD_ARG and "capture" in str(exc.value), str(exc.value)
    assert not fm.graph_pinned and bool((out == 7.0).all()), "a refused call must launch nothing"
    del refused
    release_captured(fm)  # (the Python handle was noted when the capture began)
    want = fm.process_batch_device(c, p)
    torch.cuda.synchronize()
    assert np.array_equal(np.isnan(_np(want)[..., 0]), g.gated)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            got = fm.process_batch_device(c, p)
    got.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(got, want)
    assert fm.graph_pinned
    with pytest.raises(MofError) as exc:
        fm.set_min_response(0.0)
    assert exc.value.code == _capi.MOF_ERR_BUSY and fm.min_response == g.v
    with pytest.raises(MofError) as exc:  # a larger batch would move the buffer under the graph
        fm.process_batch_device(c.repeat(2, 1, 1), p.repeat(2, 1, 1))
    assert exc.value.code == _capi.MOF_ERR_BUSY and "graph" in str(exc.value)
    del graph
    release_captured(fm)
    assert not fm.graph_pinned
    fm.set_min_response(0.0)
    assert fm.min_response == 0.0


# ---- 12. the setter ----
def test_setter_validation(gpu):
    fm = FftMethod(sample_point_size=64, max_px_speed=Q.SPEED, frame_shape=(64, 64), grid=(1, 1))
    assert fm.min_response == 0.0
    fm.set_min_response(0.25)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(MofError) as exc:
            fm.set_min_response(bad)
        assert exc.value.code == _capi.MOF_ERR_BAD_ARG and fm.min_response == 0.25
    fm.reset()
    assert fm.min_response == 0.25
    lib = _capi.load()
    assert lib.mof_fft_set_min_response(None, 0.5) == _capi.MOF_ERR_NOT_INIT and lib.mof_fft_min_response(None) == 0.0
    with pytest.raises(MofError) as exc:
        FftMethod(sample_point_size=64, frame_shape=(64, 64), grid=(1, 1), min_response=-0.5)
    assert exc.value.code == _capi.MOF_ERR_BAD_ARG


# ---- 13. the geometry tails, end to end ----
CAM = (340.0, 338.5, 376.0, 240.0, -0.28, 0.07, 0.0004, -0.0003, -0.006)  # fx, fy, cx, cy, k1, k2, p1, p2, k3 (test_geometry.py)


def test_long_range_into_get_2dt(gpu):
    """The long-range shifts into get_2dt_batch_device: armed, the unrelated pairs have no valid point left and report what the host form
    reports on the same NaN shifts; unarmed they report MOF_GEOM_OK and a velocity made of a wrong shift"""
    g = GC.long_range()
    fm = FftMethod(128, 32, Q.SPEED)
    c, p = torch.tensor(g.cur, device=gpu), torch.tensor(g.prev, device=gpu)
    lay, cam = G.Layout(1, 1, 0, 0, 32, 32, 32), G.Camera(*CAM)
    par = np.tile(np.array([[2.5, 0.02, 0.0, 0.0, 0.3]]), (4, 1))
    d_par = torch.tensor(par, device=gpu)
    unarmed = _np(G.get_2dt_batch_device(fm.process_long_range_batch_device(c, p), lay, cam, d_par))
    fm.set_min_response(g.v)
    shifts = fm.process_long_range_batch_device(c, p)
    armed = _np(G.get_2dt_batch_device(shifts, lay, cam, d_par))
    shifts = _np(shifts)
    for k in range(4):
        st, tran, diff = G.get_2dt(shifts[k], lay, cam, G.T2dParams(*par[k]))
        assert int(armed[k, 6]) == st and int(unarmed[k, 6]) == 0 and np.isfinite(unarmed[k, :3]).all(), (k, armed[k], unarmed[k], st)
        assert (st != 0) == bool(g.gated[k, 0]), (k, st)
        if st == 0:
            assert np.allclose(armed[k, :3], tran, rtol=0, atol=1e-9) and _same_bits(armed[k], unarmed[k])


def test_get_rt_on_gated_shifts(gpu):
    """One 480 x 480 pair, 4 x 4 patches of 120, five of them unrelated: get_rt_batch_device on the armed shifts is the host form on the
    same shifts (1e-9, test_gpu_geometry.py); 11 valid points are left, at least shifted_pts_thr = 8"""
    g = GC.rt480()
    fm = FftMethod(480, 120, Q.SPEED, min_response=g.v)
    shifts = fm.process_batch_device(torch.tensor(g.cur, device=gpu), torch.tensor(g.prev, device=gpu))
    lay, cam = G.reference_layout(480, 120), G.Camera(*CAM)
    par = G.RtParams(2.5, 0.02, 136.0, (C.c_double * 4)(0, 0, 0, 1), (C.c_double * 4)(0, 0, 0, 1), (C.c_double * 3)(0, 0, 0))
    d_par = torch.from_numpy(np.frombuffer(bytes(par), dtype=np.float64, count=G.RT_PARAMS_DOUBLES).reshape(1, -1).copy()).to(gpu)
    got = _np(G.get_rt_batch_device(shifts, lay, cam, d_par, 8))
    s = _np(shifts)
    assert np.array_equal(np.isnan(s[0, :, 0]), g.gated[0]) and int(np.isfinite(s[0, :, 0]).sum()) == 11
    st, rot, tran, _, _ = G.get_rt(s[0], lay, cam, par, 8)
    print(f"getRT on 11 of 16 points: status {st} ({G.STATUS.get(st)})")
    assert int(got[0, 7]) == st and st != 2, (got[0], st)  # (2: too few points)
    assert np.allclose(got[0, :4], rot, rtol=0, atol=1e-9) and np.allclose(got[0, 4:7], tran, rtol=0, atol=1e-9)


# ---- 14. the shard group, through ctypes ----
def test_shard_group_of_one(gpu):
    """mof_shard_fft_set_min_response on a group of one engine: the single engine's armed bits; MOF_ERR_BUSY, nothing changed, once a
    capture on the group's stream has pinned the engine"""
    g = GC.grid7()
    lib = _capi.load()
    fm = _engine(g, min_response=g.v)
    c, p = torch.tensor(g.cur, device=gpu), torch.tensor(g.prev, device=gpu)
    want = fm.process_batch_device(c, p)
    grp = C.c_void_p()
    _capi.check(lib.mof_shard_fft_create(C.byref(fm.cfg), (C.c_int * 1)(0), 1, C.byref(grp)))
    try:
        assert lib.mof_shard_fft_min_response(grp) == 0.0
        assert lib.mof_shard_fft_set_min_response(grp, float("nan")) == _capi.MOF_ERR_BAD_ARG and lib.mof_shard_fft_min_response(grp) == 0.0
        _capi.check(lib.mof_shard_fft_set_min_response(grp, g.v))
        assert lib.mof_shard_fft_min_response(grp) == g.v
        out = torch.zeros((7, 6, 2), dtype=torch.float64, device=gpu)
        pc, pp, po = ((C.c_void_p * 1)(t.data_ptr()) for t in (c, p, out))
        args = (grp, pc, c.stride(0), pp, p.stride(0), c.stride(1), 7, po, 0)
        torch.cuda.synchronize()
        _capi.check(lib.mof_shard_fft_process_batch_device(*args))
        _capi.check(lib.mof_shard_fft_sync(grp))
        assert _same_bits(out, want)
        ext = torch.cuda.ExternalStream(int(lib.mof_shard_fft_stream(grp, 0)), device=gpu)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(ext):
            with torch.cuda.graph(graph, stream=ext):
                _capi.check(lib.mof_shard_fft_process_batch_device(*args))
        assert lib.mof_shard_fft_set_min_response(grp, 0.0) == _capi.MOF_ERR_BUSY and lib.mof_shard_fft_min_response(grp) == g.v
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(out, want)
        del graph
    finally:
        lib.mof_shard_fft_destroy(grp)  # (a pinned engine is parked ...)
        lib.mof_purge_deferred()        # (... until its graphs are gone)


# ---- 15. the C++ mirror ----
def test_cpp_mirror(gpu, tmp_path):
    """mof::FftMethod::setMinResponse / minResponse (and ShardedFftMethod's pass-through) in tests/cpp_gate/test_fft_gate: pairs 0, 3 and 4
    of the 8 x 8 grid of 32-pixel patches through two processImage calls (previous, current) print the Python binding's armed bits"""
    assert os.path.exists(BIN), "tests/cpp_gate/test_fft_gate missing: run __graft_entry__.build()"
    g = GC.index320()
    ks = [0, 3, 4]
    path = tmp_path / "pairs.u8"
    np.concatenate([g.cur[ks], g.prev[ks]]).tofile(path)
    r = subprocess.run([BIN, "256", "32", repr(Q.SPEED), repr(g.v), str(len(ks)), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "setter ok", lines[0]
    fm = FftMethod(256, 32, Q.SPEED, min_response=g.v)
    for t, k in enumerate(ks):
        tok = lines[1 + t].split()
        assert tok[:3] == ["pair", str(t), "invalid"], tok[:4]
        fm.processImage(g.prev[k])
        s = fm.processImage(g.cur[k])
        vals = np.array([float(x) for x in tok[4:]]).reshape(64, 4)
        assert int(tok[3]) == fm.last_invalid == int(g.gated[k].sum()), (k, tok[3], fm.last_invalid)
        # (17 digits round-trip every finite double; a printed NaN carries no payload, so NaN is compared as NaN)
        assert np.array_equal(vals[:, :2], s, equal_nan=True) and np.array_equal(vals[:, 2:], fm.last_quality, equal_nan=True), k
        assert np.array_equal(np.isnan(s[:, 0]), g.gated[k])


def test_cpp_adapter_mirror(gpu, tmp_path):
    """MofFftMethod::setMinResponse / minResponse, the drop-in adapter's pass-through, in tests/cpp_gate/test_gate_adapter.cpp: the same
    three pairs through OpticFlowCalc::processImage on an armed adapter print the Python binding's armed vectors, NaN where the oracle
    gates. The binary needs the reference's interface header: oracle/gate_adapter.mk (run by tests/cpp_gate/Makefile, part of
    __graft_entry__.build()) builds it into oracle/_ref/ where the reference checkout exists, and it travels from there -- as
    test_gpu_cpp_host.py's adapter test has it."""
    binary = os.path.join(ROOT, "oracle", "_ref", "test_gate_adapter")
    assert os.path.exists(binary), "oracle/_ref/test_gate_adapter missing: run __graft_entry__.build() where the reference checkout exists"
    g = GC.index320()
    ks = [0, 3, 4]
    path = tmp_path / "pairs.u8"
    np.concatenate([g.cur[ks], g.prev[ks]]).tofile(path)
    r = subprocess.run([binary, "256", "32", repr(Q.SPEED), repr(g.v), str(len(ks)), str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "setter ok", lines[0]
    fm = FftMethod(256, 32, Q.SPEED, min_response=g.v)
    for t, k in enumerate(ks):
        tok = lines[1 + t].split()
        assert tok[:4] == ["pair", str(t), "n", "64"], tok[:4]
        fm.processImage(g.prev[k])
        s = fm.processImage(g.cur[k])
        vals = np.array([float(x) for x in tok[4:]]).reshape(64, 2)
        assert np.array_equal(np.isnan(vals[:, 0]), g.gated[k]) and np.array_equal(np.isnan(vals[:, 1]), g.gated[k]), k
        assert np.array_equal(vals, s, equal_nan=True), k  # (17 digits round-trip every finite double)


def test_stateful_entries_without_a_quality_pointer(gpu):
    """mof_fft_process and mof_fft_process_long_range (no quality pointer) on an armed engine, through ctypes: the gate reads the
    engine's own quality buffer, which the kernels must fill although the caller did not ask for it -- the shifts and n_invalid of the
    _q entries on the same frames. The buffer is first filled by a MATCHED pair through the _q entry, so a gate that read stale
    responses would pass every patch of the unrelated pair that follows."""
    lib = _capi.load()
    g = GC.grid7()
    k = next(k for k in range(7) if not g.invalid[k].any())
    m = next(m for m in range(7) if m != k and not g.unrelated[m, k % 6])  # (a pair whose patch k mod 6 is matched)

    def run(fm, entry, frames, n):
        outs = []
        for f in frames:
            out, ninv = np.full((n, 2), 7.0), C.c_int(-1)
            _capi.check(entry(fm._h, f.ctypes.data, f.strides[0], out.ctypes.data, C.byref(ninv)))
            outs.append((out, ninv.value))
        return outs

    frames = [np.ascontiguousarray(f) for f in (g.prev[m], g.cur[m], g.prev[k], g.cur[k])]
    armed, ref = _engine(g, min_response=g.v), _engine(g, min_response=g.v)
    want = [(ref.processImage(f), ref.last_invalid) for f in frames]
    got = [(armed.processImage(f), armed.last_invalid) for f in frames[:2]] + run(armed, lib.mof_fft_process, frames[2:], 6)
    for (out, ninv), (w, winv) in zip(got, want):
        assert _same_bits(out, w) and ninv == winv, (out, w)
    assert np.flatnonzero(np.isnan(got[3][0][:, 0])).tolist() == [k % 6] and got[3][1] == 1
    assert not np.isnan(got[1][0][k % 6]).any()
    # the long-range entry: pair 0 matched, pair 1 against an unrelated frame
    lr = GC.long_range()
    frames = [np.ascontiguousarray(f) for f in (lr.prev[0], lr.cur[0], lr.prev[1], lr.cur[1])]
    armed, ref = FftMethod(128, 32, Q.SPEED, min_response=lr.v), FftMethod(128, 32, Q.SPEED, min_response=lr.v)
    want = [(ref.processImageLongRange(f), ref.last_invalid) for f in frames]
    got = [(armed.processImageLongRange(f), armed.last_invalid) for f in frames[:2]] + run(armed, lib.mof_fft_process_long_range, frames[2:], 1)
    for (out, ninv), (w, winv) in zip(got, want):
        assert _same_bits(out, w) and ninv == winv, (out, w)
    assert np.isfinite(got[1][0]).all() and np.isnan(got[3][0]).all() and got[3][1] == 1
