"""Three block matchers of different routes alive at once on one thread and called in rotation: each engine launches by the route it was
created with (csrc/mof_kernels.h, BmRoute), whatever the engine called before it launched.

  s16   16 x 16, step 8, radius 4 on 96 x 128: scan16
  g16   16 x 16, step 0, radius 3 on 96 x 96: the generic scan at 16 (odd radius)
  g32   32 x 32, step 0, radius 8 on 96 x 96: the generic scan, c1's class

Per engine three stateful frames and one batch of three pairs, each plain, with the quality outputs, and with the match gate armed. Every
output equals the CPU oracle's (tests/bm_quality_cases.py: integers, exact equality) and what a fresh engine of the same geometry gives
when it is the only one. A route kept in a static or per thread, not in the engine, fails here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bm_quality_cases as BQ
from mrs_optic_flow_amd import _capi

pytestmark = pytest.mark.gpu
OFF = 0xFFFFFFFF


class _Shape(BQ.Shape):
    """A FastSpacedBMMethod geometry on a given frame (BQ.Shape derives the frame from the grid)"""

    def __init__(self, name, block, radius, step, hw, scan16):
        S = block + step
        super().__init__(name, block, radius, step, ((hw[1] - 2 * radius) // S, (hw[0] - 2 * radius) // S), scan16)
        self.h, self.w = hw


SHAPES = (_Shape("s16", 16, 4, 8, (96, 128), True), _Shape("g16", 16, 3, 0, (96, 96), False), _Shape("g32", 32, 8, 0, (96, 96), False))
STEPS = tuple((entry, form) for entry in ("stateful", "batch") for form in ("plain", "quality", "gate"))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(shape, the scenes batch, the same frames as a sequence prev0, cur0, cur2, cur1 with the oracle of its three consecutive pairs, gate)"""
    s = next(s for s in SHAPES if s.name == name)
    cur, prev = BQ._scenes(s)
    b = BQ.Batch(s, "scenes", cur, prev)
    frames = np.stack([prev[0], cur[0], cur[2], cur[1]])
    seq = BQ.Batch(s, "scenes", frames[1:], frames[:-1])
    a, r, _ = b.thresholds()
    return s, b, frames, seq, (a, r)


def _stateful(eng, s, frames, want_q):
    """setImPrev(frames[0]), then every other frame through the stateful entry: (dx, dy, mode_xy[, quality, n_invalid]) stacked over the frames"""
    lib = _capi.load()
    eng.setImPrev(frames[0])
    out = []
    for f in frames[1:]:
        f = np.ascontiguousarray(f)
        dx, dy, mode = np.full(s.blocks, 99, np.int8), np.full(s.blocks, 99, np.int8), np.full(2, 99, np.int8)
        if want_q:
            q, n = np.full((s.grid[1], s.grid[0], 3), 99, np.uint32), C.c_int(99)
            _capi.check(lib.mof_bm_process_q(eng._h, f.ctypes.data, f.strides[0], dx.ctypes.data, dy.ctypes.data, mode.ctypes.data, q.ctypes.data,
                                             C.byref(n)))
            out.append((dx.reshape(s.grid[::-1]), dy.reshape(s.grid[::-1]), mode, q, np.int32(n.value)))
        else:
            _capi.check(lib.mof_bm_process(eng._h, f.ctypes.data, f.strides[0], dx.ctypes.data, dy.ctypes.data, mode.ctypes.data))
            out.append((dx.reshape(s.grid[::-1]), dy.reshape(s.grid[::-1]), mode))
    return tuple(np.stack(a) for a in zip(*out))


def _step(eng, case, dev, entry, form):
    """One step on one engine: (what it returned, what the oracle says)"""
    s, b, frames, seq, gate = case
    a, r = gate if form == "gate" else (OFF, 0)
    eng.set_gate(None if a == OFF else a, r)
    ref = seq if entry == "stateful" else b
    wdx, wdy, wmode, wn = ref.gated(a, r)
    if entry == "stateful":
        got = _stateful(eng, s, frames, form != "plain")
        want = (wdx, wdy, wmode[:, :2]) + ((ref.quality, wn) if form != "plain" else ())
    else:
        c, p = dev
        if form == "plain":
            got = tuple(t.cpu().numpy() for t in eng.process_batch_device(c, p))
            want = (wdx, wdy, wmode)
        else:
            dx, dy, mode, (q, n) = eng.process_batch_device(c, p, return_quality=True)
            got = (dx.cpu().numpy(), dy.cpu().numpy(), mode.cpu().numpy(), q.cpu().numpy().view(np.uint32), n.cpu().numpy())
            want = (wdx, wdy, wmode, ref.quality, wn)
    return got, want


def _same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, k, g, w)


@functools.lru_cache(maxsize=None)
def _alone(name):
    """every step on a fresh engine that is the only block matcher alive"""
    case = _case(name)
    dev = tuple(torch.tensor(x, device="cuda:0") for x in (case[1].cur, case[1].prev))
    eng = case[0].engine()
    out = {st: _step(eng, case, dev, *st)[0] for st in STEPS}
    eng.close()
    return out


def test_routes_are_the_three_classes(gpu):
    lib = _capi.load()
    for s in SHAPES:
        plan = (C.c_int * 4)()
        _capi.check(lib.mof_bm_scan_plan(s.block, s.step, s.radius, s.grid[0], 0, plan))
        assert bool(plan[0]) == s.scan16, (s.name, tuple(plan))


def test_three_engines_in_rotation(gpu):
    alone = {s.name: _alone(s.name) for s in SHAPES}
    cases = {s.name: _case(s.name) for s in SHAPES}
    devs = {n: tuple(torch.tensor(x, device=gpu) for x in (c[1].cur, c[1].prev)) for n, c in cases.items()}
    engines = {s.name: s.engine() for s in SHAPES}
    for st in STEPS:
        for name, eng in engines.items():
            got, want = _step(eng, cases[name], devs[name], *st)
            _same(got, want, f"{name} {st}: against the oracle")
            _same(got, alone[name][st], f"{name} {st}: against the engine used alone")
    # ... and once more in the other order, the gate left armed by the last step switched off again
    for st in reversed(STEPS):
        for name in reversed(list(engines)):
            got, want = _step(engines[name], cases[name], devs[name], *st)
            _same(got, want, f"{name} {st}, reversed: against the oracle")
    for eng in engines.values():
        eng.close()
