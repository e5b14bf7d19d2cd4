"""The block matchers' per-block SAD quality {min_sad, zero_sad, max_sad} and the opt-in match gate, on the GPU, against the CPU oracle.

Inputs, shapes and references: tests/bm_quality_cases.py (test_bm_quality_host.py shows on the oracle that the inputs are what they claim).
Everything is integer: every comparison below is exact equality."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import bm_quality_cases as BQ
from mrs_optic_flow_amd import BlockMethod, _capi
from mrs_optic_flow_amd._capi import MofError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp_bm_quality", "test_bm_quality")
OFF = 0xFFFFFFFF


def _dev(b, gpu):
    return torch.tensor(b.cur, device=gpu), torch.tensor(b.prev, device=gpu)


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _run_q(eng, c, p):
    dx, dy, mode, (q, n) = eng.process_batch_device(c, p, return_quality=True)
    dx, dy, mode, q, n = _np(dx, dy, mode, q, n)
    return dx, dy, mode, q.view(np.uint32), n


def _holds(got, want, what):
    for name, g, w in zip(("dx", "dy", "mode", "quality", "n_invalid"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


def _check_gate(eng, b, c, p, a, r, what):
    """arm (a, r): the _q entry and the plain entry against the oracle's gated outputs; the quality is the ungated one"""
    eng.set_gate(None if a == OFF else a, r)
    assert eng.gate == (None if a == OFF else a, r)
    want = b.gated(a, r)
    got = _run_q(eng, c, p)
    _holds(got, (want[0], want[1], want[2], b.quality, want[3]), what)
    plain = _np(*eng.process_batch_device(c, p))
    _holds(plain, want[:3], what + ", entry without _q")
    return want


# ---- 1. quality on every shape and content ----
@pytest.mark.parametrize("content", BQ.CONTENTS)
@pytest.mark.parametrize("name", list(BQ.SHAPES))
def test_quality_matches_oracle(gpu, name, content):
    """The three raw SADs equal the oracle's; dx, dy and mode with the quality on are the bits of the entry without it and the oracle's"""
    b = BQ.batch(name, content)
    eng = b.shape.engine()
    plan = (C.c_int * 4)()
    _capi.check(_capi.load().mof_bm_scan_plan(b.shape.block, b.shape.step, b.shape.radius, b.shape.grid[0], 1, plan))
    print(f"route {name}: scan16 {plan[0]} bpw {plan[1]} threads {plan[2]} lds {plan[3]}")
    if not os.environ.get("MOF_BM_GENERIC"):
        assert bool(plan[0]) == b.shape.scan16
    c, p = _dev(b, gpu)
    plain = _np(*eng.process_batch_device(c, p))
    _holds(plain, (b.dx, b.dy, b.mode), f"{name} {content}, plain")
    got = _run_q(eng, c, p)
    _holds(got, (b.dx, b.dy, b.mode, b.quality, np.zeros(len(b.cur), np.int32)), f"{name} {content}")
    # the quality pointer alone, the count alone (the gated mode kernel, unarmed: bm_mode_kernel's bytes)
    lib, n = _capi.load(), len(b.cur)
    dx, dy, mode = (torch.full(a.shape, 99, dtype=torch.int8, device=gpu) for a in (b.dx, b.dy, b.mode))
    cnt = torch.full((n,), 99, dtype=torch.int32, device=gpu)
    _capi.check(lib.mof_bm_process_batch_device_q(eng._h, c.data_ptr(), c.stride(0), p.data_ptr(), p.stride(0), c.stride(1), n, dx.data_ptr(),
                                                  dy.data_ptr(), mode.data_ptr(), None, cnt.data_ptr(), None))
    torch.cuda.synchronize()
    _holds(_np(dx, dy, mode, cnt), (b.dx, b.dy, b.mode, np.zeros(n, np.int32)), f"{name} {content}, count only")


# ---- 2. the gate on the mixed scenes ----
@pytest.mark.parametrize("name", list(BQ.SHAPES))
def test_gate_on_mixed_scenes(gpu, name):
    """Thresholds inside the oracle's gap: each measure alone, both together, and off again"""
    b = BQ.batch(name, "scenes")
    a, r, figures = b.thresholds()
    print(f"gates {name}: max_min_sad {a} min_sad_range {r} from {figures}")
    eng = b.shape.engine()
    c, p = _dev(b, gpu)
    for thr in ((a, 0), (OFF, r), (a, r)):
        want = _check_gate(eng, b, c, p, *thr, f"{name} gate {thr}")
        assert want[3][0] == 0 and want[3][1] == b.shape.blocks  # matched pair untouched, unrelated pair gated whole
        assert (want[2][1, :6] == BQ.INVALID).all() and (want[2][:, 6:] == 0).all()
    eng.set_gate(None, 0)
    assert eng.gate == (None, 0)
    _holds(_run_q(eng, c, p), (b.dx, b.dy, b.mode, b.quality, np.zeros(3, np.int32)), f"{name} disarmed")


@pytest.mark.parametrize("name", ["s16-r8", "g8-r3"])
def test_threshold_edges(gpu, name):
    """max_min_sad equal to a block's min_sad passes it, one less gates it; min_sad_range equal to its range passes it, one more gates it"""
    b = BQ.batch(name, "scenes")
    q = b.quality.astype(np.int64)[2].reshape(-1, 3)
    blk = int(np.argmax(q[:, 0]))  # the mixed pair's worst block
    m, rg = int(q[blk, 0]), int(q[blk, 2] - q[blk, 0])
    eng = b.shape.engine()
    c, p = _dev(b, gpu)
    for a, r, passes in ((m, 0, True), (m - 1, 0, False), (OFF, rg, True), (OFF, rg + 1, False), (m, rg, True)):
        assert bool(b.valid(a, r)[2].reshape(-1)[blk]) == passes
        _check_gate(eng, b, c, p, a, r, f"{name} edge ({a}, {r})")


def test_constant_pair_on_block_method(gpu):
    """BlockMethod has no validity rule: on a constant pair every block reports (-r, -r) and so does the mode; with min_sad_range = 1
    every block is invalid, the mode is MOF_BM_INVALID six times, n_invalid = blocks, and processImage returns no vector"""
    cur, prev = BQ.constant_block_method()
    bm = BlockMethod(52, 16, 2)
    blocks = bm.n_blocks
    assert blocks == 9
    c, p = torch.tensor(cur, device=gpu), torch.tensor(prev, device=gpu)
    dx, dy, mode, q, n = _run_q(bm, c, p)
    assert (dx == -2).all() and (dy == -2).all() and list(mode[0]) == [-2, -2, -1, -1, 0, 0, 0, 0] and n[0] == 0 and (q == 0).all()
    bm.set_gate(None, 1)
    dx, dy, mode, q, n = _run_q(bm, c, p)
    assert (dx == BQ.INVALID).all() and (dy == BQ.INVALID).all() and list(mode[0]) == [BQ.INVALID] * 6 + [0, 0] and n[0] == blocks and (q == 0).all()
    bm.setImPrev(prev[0])
    out = bm.processImage(cur[0], refine="faithful")
    assert out.shape == (1, 2) and np.isnan(out).all() and bm.last_n_invalid == blocks
    bm.set_gate(None, 0)
    assert np.array_equal(bm.processImage(cur[0]), [[-2.0, -2.0]]) and bm.last_n_invalid == 0


def test_low_contrast_rule_with_the_gate(gpu):
    """FastSpacedBMMethod's rule runs first and a block it zeroed still votes when it is valid: a nearly flat pair (the rule zeroes every
    block) with two windows of prev replaced by an unrelated view (gated by max_min_sad)"""
    s = BQ.SHAPES["s16-r8"]
    rng = np.random.default_rng(41)
    cur = (100 + (rng.random((1, s.h, s.w)) < 0.05)).astype(np.uint8)
    prev = (100 + (rng.random((1, s.h, s.w)) < 0.05)).astype(np.uint8)
    for blk in (3, 20):
        y, x, n = s.window(blk)
        prev[0, y:y + n, x:x + n] = BQ.GC.unrelated(n, n, 42 + blk)
    b = BQ.Batch(s, "flat", cur, prev)
    q = b.quality.astype(np.int64).reshape(-1, 3)
    a = 16 * 16 * 8  # 8 grey levels per pixel: far above the flat blocks, far below the replaced ones
    v = b.valid(a, 0).reshape(-1)
    zeroed = (q[:, 0] < q[:, 1]) & (b.dx.reshape(-1) == 0) & (b.dy.reshape(-1) == 0)  # the raw minimum is not the centre, the rule moved it there
    assert (zeroed & v).any() and (~v).sum() >= 2 and not v[3] and not v[20]
    eng = s.engine()
    want = _check_gate(eng, b, *_dev(b, gpu), a, 0, "low-contrast rule under the gate")
    assert tuple(want[2][0, :2]) == (0, 0)


# ---- 3. each entry once ----
def test_stateful_entries(gpu):
    """mof_bm_process_q through processBlocks (last_quality, last_n_invalid), mof_bm_process with the gate armed, the frame chain"""
    b = BQ.batch("g12-r5", "scenes")
    a, r, _ = b.thresholds()
    want = b.gated(a, r)
    eng = b.shape.engine(max_min_sad=a, min_sad_range=r)
    assert eng.gate == (a, r)
    lib, nb = _capi.load(), b.shape.blocks
    for k in range(3):
        eng.setImPrev(b.prev[k])
        dx, dy, mode = eng.processBlocks(b.cur[k])
        _holds((dx, dy, np.array(mode, np.int8), eng.last_quality, np.int32(eng.last_n_invalid)),
               (want[0][k], want[1][k], want[2][k, :2], b.quality[k], want[3][k]), f"stateful pair {k}")
        eng.setImPrev(b.prev[k])
        pdx, pdy, pm = np.empty(nb, np.int8), np.empty(nb, np.int8), np.zeros(2, np.int8)
        f = b.cur[k]
        _capi.check(lib.mof_bm_process(eng._h, f.ctypes.data, f.strides[0], pdx.ctypes.data, pdy.ctypes.data, pm.ctypes.data))
        assert np.array_equal(pdx, want[0][k].ravel()) and np.array_equal(pdy, want[1][k].ravel()) and np.array_equal(pm, want[2][k, :2])
    # the chain: the frame of a fully gated call still becomes the previous one
    eng.set_gate(None, OFF)
    assert np.isnan(eng.processImage(b.prev[0])).all() and eng.last_n_invalid == nb
    eng.set_gate(None, 0)
    dx, dy, mode = eng.processBlocks(b.cur[0])
    assert np.array_equal(dx, b.dx[0]) and np.array_equal(dy, b.dy[0]) and mode == tuple(b.mode[0, :2]) and np.array_equal(eng.last_quality, b.quality[0])


@pytest.mark.parametrize("name", ["s16-r8", "g32-r8"])
def test_bgr_entry(gpu, name):
    cur, prev, b = BQ.bgr_scenes(name)
    a, r, _ = b.thresholds()
    want = b.gated(a, r)
    eng = b.shape.engine(max_min_sad=a, min_sad_range=r)
    c, p = torch.tensor(cur, device=gpu), torch.tensor(prev, device=gpu)
    dx, dy, mode, (q, n) = eng.process_batch_device_bgr(c, p, return_quality=True)
    _holds(_np(dx, dy, mode) + (q.cpu().numpy().view(np.uint32), n.cpu().numpy()), (want[0], want[1], want[2], b.quality, want[3]), f"{name} BGR8")
    _holds(_np(*eng.process_batch_device_bgr(c, p)), want[:3], f"{name} BGR8 without _q")


def test_host_entry(gpu):
    """mof_bm_process_batch_host_q and the entry without _q, armed (test_host_entry_in_chunks runs it with the batch split)"""
    b = BQ.batch("s16-r6", "scenes")
    a, r, _ = b.thresholds()
    want = b.gated(a, r)
    eng = b.shape.engine(max_min_sad=a, min_sad_range=r)
    print(f"route host: chunk {os.environ.get('MOF_HOST_CHUNK', 'default')}")
    dx, dy, mode, (q, n) = eng.process_batch_host(b.cur, b.prev, return_quality=True)
    _holds((dx, dy, mode, q, n), (want[0], want[1], want[2], b.quality, want[3]), "host _q")
    _holds(eng.process_batch_host(b.cur, b.prev), want[:3], "host")
    # the count alone: no quality read-back
    lib = _capi.load()
    n2 = np.full(3, 99, np.int32)
    _capi.check(lib.mof_bm_process_batch_host_q(eng._h, b.cur.ctypes.data, b.cur.strides[0], b.prev.ctypes.data, b.prev.strides[0],
                                                b.cur.strides[1], 3, dx.ctypes.data, dy.ctypes.data, mode.ctypes.data, None, n2.ctypes.data))
    _holds((dx, dy, mode, n2), (want[0], want[1], want[2], want[3]), "host, count only")


_DIED = []  # a child that ended on a signal or at its time limit: no later test starts another on the same card


def _child(env, select, passed, expect):
    if _DIED:
        pytest.fail(f"not started: an earlier child of this module died ({_DIED[0]}); find its cause first")
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-s", "-k", select, "-p", "no:cacheprovider"],
                           capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, **env))
    except subprocess.TimeoutExpired:
        _DIED.append(f"{env}: no end within 300 s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DIED.append(f"{env}: status {r.returncode}")
    for line in r.stdout.splitlines():
        if "route " in line or "gates " in line or " passed" in line:
            print(f"[{' '.join(f'{k}={v}' for k, v in env.items())}] {line}")
    assert r.returncode == 0 and f"{passed} passed" in r.stdout and " skipped" not in r.stdout, (env, r.returncode, r.stdout[-3000:], r.stderr[-1500:])
    for text in expect:
        assert text in r.stdout + r.stderr, (env, text, r.stdout[-2000:], r.stderr[-1500:])


def test_host_entry_in_chunks(gpu):
    """MOF_HOST_CHUNK=2 (read once per process): the three pairs go up as 2 + 1"""
    _child({"MOF_HOST_CHUNK": "2"}, "test_host_entry and not chunks", 1, ["route host: chunk 2"])


@pytest.mark.parametrize("name,env", BQ.KNOBS, ids=[f"{n}-{'-'.join(f'{k}={v}' for k, v in e.items())}" for n, e in BQ.KNOBS])
def test_knob_routes(gpu, name, env):
    """The quality form and the gate on the routes only a knob selects: block 16 / radius 8 on the generic scan, block 32 / radius 8 with
    one, two and three groups of four x-shifts per lane, and block 100 / radius 4 on the one plan whose quality form has to take one block
    fewer per workgroup to stay inside the LDS (the plan line of MOF_BM_VERBOSE names the route taken)"""
    xb = env.get("MOF_BM_XB")
    expect = [f"route {name}: scan16 0", f"block scan plan xb {xb} " if xb else "block scan plan xb "]
    if name == "g100-r4":  # the plain plan's 7 blocks per workgroup and the quality form's 6, both launched
        expect += ["route g100-r4: scan16 0 bpw 6 ", "bpw 7 wpd", "bpw 6 wpd"]
    _child(dict(env, MOF_BM_VERBOSE="1"), f"(test_quality_matches_oracle or test_gate_on_mixed_scenes) and {name}", 4, expect)


def test_shard_group_of_one(gpu):
    """mof_shard_bm_set_gate on a group of one engine: the slab keeps its layout and holds the single engine's armed bits"""
    b = BQ.batch("s16-r6", "scenes")
    a, r, _ = b.thresholds()
    want = b.gated(a, r)
    eng = b.shape.engine()
    lib, nb = _capi.load(), b.shape.blocks
    c, p = _dev(b, gpu)
    grp = C.c_void_p()
    _capi.check(lib.mof_shard_bm_create(C.byref(eng.cfg), (C.c_int * 1)(0), 1, C.byref(grp)))
    try:
        ga, gb = C.c_uint32(7), C.c_uint32(7)
        _capi.check(lib.mof_shard_bm_gate(grp, C.byref(ga), C.byref(gb)))
        assert (ga.value, gb.value) == (OFF, 0)
        _capi.check(lib.mof_shard_bm_set_gate(grp, a, r))
        _capi.check(lib.mof_shard_bm_gate(grp, C.byref(ga), C.byref(gb)))
        assert (ga.value, gb.value) == (a, r)
        slab = lib.mof_shard_bm_slab_bytes(grp, 3)
        assert slab == (3 * (2 * nb + 8) + 15) // 16 * 16
        out = torch.zeros(slab, dtype=torch.int8, device=gpu)
        pc, pp, po = ((C.c_void_p * 1)(t.data_ptr()) for t in (c, p, out))
        torch.cuda.synchronize()
        _capi.check(lib.mof_shard_bm_process_batch_device(grp, pc, c.stride(0), pp, p.stride(0), c.stride(1), 3, po, 0))
        _capi.check(lib.mof_shard_bm_sync(grp))
        got = out.cpu().numpy()
        assert np.array_equal(got[:3 * nb], want[0].ravel()) and np.array_equal(got[3 * nb:6 * nb], want[1].ravel())
        assert np.array_equal(got[6 * nb:6 * nb + 24], want[2].ravel())
    finally:
        lib.mof_shard_bm_destroy(grp)


# ---- 4. the setter ----
def test_setter_contract(gpu):
    """The default reads back as (UINT32_MAX, 0); MOF_ERR_BUSY while a call is in flight, and then nothing has changed; disarming restores
    the ungated bytes (test_gate_on_mixed_scenes ends on that for every shape)"""
    b = BQ.batch("g32-r8", "scenes")
    eng = b.shape.engine()
    lib = _capi.load()
    ga, gb = C.c_uint32(7), C.c_uint32(7)
    _capi.check(lib.mof_bm_gate(eng._h, C.byref(ga), C.byref(gb)))
    assert (ga.value, gb.value) == (OFF, 0) and eng.gate == (None, 0)
    with pytest.raises(ValueError):
        eng.set_gate(-1, 0)
    assert eng.gate == (None, 0)
    # a second thread keeps stateful calls in flight (each holds the engine from its upload to its read-back)
    done = threading.Event()

    def work():
        try:
            for k in range(200):
                try:
                    eng.processBlocks(b.cur[k % 3])
                except MofError as e:  # the setter held the engine for a moment
                    assert e.code == _capi.MOF_ERR_BUSY
        finally:
            done.set()

    t = threading.Thread(target=work)
    current, busy, flips = (OFF, 0), 0, 0
    t.start()
    while not done.is_set():
        nxt = (1000 + flips, 5 + flips)
        rc = lib.mof_bm_set_gate(eng._h, *nxt)
        if rc == _capi.MOF_OK:
            current, flips = nxt, flips + 1
        else:
            assert rc == _capi.MOF_ERR_BUSY
            busy += 1
        _capi.check(lib.mof_bm_gate(eng._h, C.byref(ga), C.byref(gb)))
        assert (ga.value, gb.value) == current  # a refused call changed nothing
    t.join()
    print(f"setter: {busy} busy answers, {flips} accepted")
    assert busy > 0
    with pytest.raises(MofError) as exc:
        _capi.check(lib.mof_bm_set_gate(None, 1, 1))
    assert exc.value.code == _capi.MOF_ERR_NOT_INIT


# ---- 5. the C++ mirror ----
def test_cpp_mirror(gpu, tmp_path):
    """mof::BlockMatcherBase::setGate / gate / lastQuality / invalidBlocks / processBatchDeviceQ and ShardedBlockMatcher::setGate in
    tests/cpp_bm_quality/test_bm_quality, against the oracle's integers"""
    assert os.path.exists(BIN), "tests/cpp_bm_quality/test_bm_quality missing: run __graft_entry__.build()"
    b = BQ.batch("s16-r6", "scenes")
    s = b.shape
    a, r, _ = b.thresholds()
    dx, dy, mode, n_invalid = b.gated(a, r)
    path = tmp_path / "frames.u8"
    path.write_bytes(b.cur.tobytes() + b.prev.tobytes())
    res = subprocess.run([BIN, str(s.block), str(s.radius), str(s.step), str(s.w), str(s.h), str(a), str(r), "3", str(path)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    lines = res.stdout.splitlines()
    assert lines[0] == "setter ok" and len(lines) == 7
    for k in range(3):
        per = np.concatenate([dx[k].reshape(-1, 1), dy[k].reshape(-1, 1), b.quality[k].reshape(-1, 3).astype(np.int64)], axis=1).ravel()
        blocks = " ".join(str(int(v)) for v in per)
        vectors = 0 if mode[k, 0] == BQ.INVALID else 1
        assert lines[1 + k] == f"stateful {k} invalid {n_invalid[k]} vectors {vectors} {blocks}", (k, lines[1 + k])
        assert lines[4 + k] == f"batch {k} invalid {n_invalid[k]} mode {' '.join(str(int(v)) for v in mode[k])} {blocks}", (k, lines[4 + k])
