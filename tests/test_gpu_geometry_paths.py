"""GPU half of the geometry-tail path tests: every case of geom_cases.py through mof_geom_get_rt_batch_device, one launch per (layout,
camera, thr), against the library's host form AND the oracle. test_geom_cases_host.py proves on the CPU that the two references agree on
every case and that the cases reach the kernel's later RANSAC rounds, its small-n branches and every exit; here the device must give

  the same status; rot and tran within 1e-9 (test_gpu_geometry.py's bar: the device libm differs from glibc in the last bits of
  acos / sin / cos / log, nothing else does -- the file is built with -ffp-contract=off; the bar is not widened for the noisy scenes);
  exactly (0, 0, 0, 1, 0, 0, 0) on every row whose status is not 0; no NaN anywhere.

What catches what (read with geom_get_rt_kernel in csrc/mof_geom.hip):
  * `i = idx % grid_x, j = idx / grid_x` with grid_y in either place: the late grids 13x5, 5x13, 17x15 and 20x13 and the 13x5 rows of small_n
    put every patch but the first row's at another centre -> a and b change -> another homography: the values leave 1e-9 (the shifts are
    those of ONE motion only at the true centres).
  * best[] not taken from the round that owns best_iter (left from an earlier round, or fetched against another base): every late
    geometry has 9 ... 24 of 32 pairs whose accepted hypothesis lies at index >= 64, all compared by value; a wrong model's mask is not
    the consensus set, so the refit (and on the noisy scenes even another full-consensus model's mask) gives other values or status 3.
    (Reading lane `best_iter` instead of `best_iter - base` is NOT a different program: __shfl masks its lane with width - 1 and base is
    a multiple of 64.)
  * the cut `base < scan.niters` / ransac_accept's `iter >= niters`: every late pair ends inside a later round (niters 239 ... 1200); a scan
    that stops a round early loses the 9 ... 24 late models of each geometry, one that ignores niters may take a later, larger consensus
    on the noisy scenes (the host form does not).
  * the ballot compaction across 64 lanes: 63 / 64 / 65 valid of 65 by position of the NaN patches, 21 valid at the end only.
  * n == 4, n < 4, n = 5 ... 7, every status 0 ... 8: small_n and exits.
  * homography_fit_wave against the one-lane homography_fit: fit_forms, bit for bit.

Measured on an MI355X (reported, not a bar): largest device - host difference late 1.1e-16, small_n 5.6e-17, exits 0, fit_forms 0; the
two fit forms agree in every bit on all 32 pairs; the whole file takes about 2 s."""
import ctypes as C

import numpy as np
import pytest
import torch

import geom_cases as GC
import oracle_lib as O
from mrs_optic_flow_amd import _capi, geometry as G

pytestmark = pytest.mark.gpu

IDENT = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
SENTINEL = -7.25e300
GUARD = 8


def run(gpu, cases, guard=0):
    """one launch over cases that share layout, camera and thr -> float64 [len(cases) + guard, 8] on the host; the guard rows hold SENTINEL
    before the launch (the C entry is called directly: the Python wrapper allocates exactly n rows)"""
    key = cases[0].key
    assert all(c.key == key for c in cases)
    lay, cam, _ = cases[0].lib_args()
    d_sh = torch.from_numpy(np.stack([c.shifts for c in cases])).to(gpu)
    d_par = torch.from_numpy(np.stack([c.param_row() for c in cases])).to(gpu)
    if not guard:
        out = G.get_rt_batch_device(d_sh, lay, cam, d_par, cases[0].thr)
    else:
        out = torch.full((len(cases) + guard, 8), SENTINEL, dtype=torch.float64, device=gpu)
        s = torch.cuda.current_stream(gpu)
        _capi.check(_capi.load().mof_geom_get_rt_batch_device(d_sh.data_ptr(), C.byref(lay), C.byref(cam), d_par.data_ptr(), len(cases),
                                                              cases[0].thr, out.data_ptr(), C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def check_rows(cases, got):
    """-> the largest device - host difference of the status-0 rows"""
    refs = GC.references()
    worst = 0.0
    assert not np.isnan(got).any(), [c.name for c, r in zip(cases, got) if np.isnan(r).any()]
    for c, row in zip(cases, got):
        (st, rot, tran, _, _), (wst, wrot, wtran, _, _) = refs[c.name]
        assert row[7] == st == wst, (c.name, row[7], st, wst)
        if st != 0:
            assert np.array_equal(row[:7], IDENT), (c.name, row)
            continue
        for r, t in ((rot, tran), (wrot, wtran)):
            assert np.allclose(row[:4], r, rtol=0, atol=1e-9) and np.allclose(row[4:7], t, rtol=0, atol=1e-9), (c.name, row, r, t)
        worst = max(worst, float(np.abs(row[:7] - np.concatenate([rot, tran])).max()))
    return worst


FAMILIES = {"late": GC.late, "small_n": GC.small_n, "exits": GC.exits, "fit_forms": lambda: GC.fit_forms()[0] + GC.fit_forms()[1]}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_case_equals_host_and_oracle(gpu, family):
    worst, statuses, launches = 0.0, set(), 0
    for cases in GC.batches(FAMILIES[family]()).values():
        got = run(gpu, cases)
        worst = max(worst, check_rows(cases, got))
        statuses |= {int(s) for s in got[:, 7]}
        launches += 1
    print(f"\n{family}: {launches} launches, statuses {sorted(statuses)}, largest device - host difference {worst:.3g}")
    if family == "exits":
        assert statuses == {0, 1, 2, 3, 4, 5, 6, 7, 8}


def test_wave_fit_equals_lane_fit_bit_for_bit(gpu):
    """the 256 / 257 boundary of kWaveFitPoints: 256 patches are refitted by homography_fit_wave, the same points in a 272-patch layout (and
    the 257-patch row of `exits`, held to the host form above) by lane 0 through homography_fit. The comment above homography_fit_wave
    promises identical results: identical bits."""
    small, padded = GC.fit_forms()
    a, b = run(gpu, list(small)), run(gpu, list(padded))
    check_rows(small, a)
    check_rows(padded, b)
    assert (a[:, 7] == 0).all()
    differ = np.flatnonzero((a.view(np.int64) != b.view(np.int64)).any(axis=1))
    assert differ.size == 0, [(small[k].name, a[k], b[k]) for k in differ[:4]]
    print(f"\nfit_forms: {len(small)} pairs, whole-wave fit == one-lane fit bit for bit")


def _failing(like, rng):
    """three pairs in `like`'s launch group that end in status 1, 2 and 3"""
    junk = rng.uniform(-like.cam[0], like.cam[0], like.shifts.shape)
    kw = dict(layout=like.layout, cam=like.cam, thr=like.thr)
    fails = [GC.Case("x", "bad duration", like.shifts, dt=0.0, **kw), GC.Case("x", "nothing valid", np.full_like(like.shifts, np.nan), **kw),
             GC.Case("x", "no consensus", junk, **kw)]
    assert [GC.host(c)[0] for c in fails] == [1, 2, 3] == [GC.oracle(c)[0] for c in fails]
    return fails


@pytest.mark.parametrize("group", ["late 13x5 noisy", "late 20x13 noisy"])     # whole-wave refit; one-lane refit
def test_a_pair_keeps_its_bits_wherever_it_stands(gpu, group):
    base = [c for c in GC.late() if c.group == group]
    assert len(base) == GC.PAIRS
    plain = run(gpu, base)
    fails = _failing(base[0], np.random.default_rng(11))
    mixed, where = [], {}
    for i, c in enumerate(reversed(base)):
        where[len(mixed)] = len(base) - 1 - i
        mixed += [c, fails[i % 3]]
    got = run(gpu, mixed)
    for pos, src in where.items():
        assert np.array_equal(got[pos].view(np.int64), plain[src].view(np.int64)), (base[src].name, got[pos], plain[src])
        assert got[pos + 1, 7] == 1 + (pos // 2) % 3 and np.array_equal(got[pos + 1, :7], IDENT), (pos, got[pos + 1])


def test_rows_beyond_n_pairs_stay_untouched(gpu):
    exits = GC.batches(GC.exits())
    mixed = max(exits.values(), key=len)                                       # the 7 x 5, thr 8 launch: statuses 0, 1, 2, 4, 5, 6, 7
    late = [c for c in GC.late() if c.group == "late 20x13 exact"]
    for cases in (mixed, late, mixed[:1]):
        got = run(gpu, cases, guard=GUARD)
        check_rows(cases, got[:len(cases)])
        assert (got[len(cases):].view(np.int64) == np.float64(SENTINEL).view(np.int64)).all(), got[len(cases):]
    assert len({int(s) for s in run(gpu, mixed)[:, 7]}) >= 6


# ---- get2DT -----------------------------------------------------------------------------------------------------------

def _2dt_inputs():
    """65 pairs on a 5 x 3 grid: only the last vector finite; inf components in front of the first usable vector; nothing usable; a
    bad duration; everything finite"""
    rng = np.random.default_rng(53)
    B, total = 65, 15
    shifts = rng.normal(0, 6, (B, total, 2))
    for k in range(B):
        if k % 4 == 0:
            shifts[k, :total - 1] = np.nan                     # the scan must reach the last patch
        elif k % 4 == 1:
            shifts[k, :5, k % 2] = np.inf if k % 8 == 1 else -np.inf        # one infinite component makes the vector unusable
            shifts[k, 5, 1 - k % 2] = np.nan
        elif k % 4 == 2:
            shifts[k, 0] = np.nan
    shifts[6] = np.nan
    shifts[62, :, 0] = np.inf                                  # nothing usable: status 2
    vals = np.stack([rng.uniform(0.5, 9, B), rng.uniform(0.002, 0.1, B), rng.normal(0, 0.4, B), rng.normal(0, 0.4, B),
                     rng.uniform(-3.2, 3.2, B)], axis=1)
    vals[9, 1] = 0.0
    vals[63, 1] = -0.0
    vals[64, 1] = np.nan
    return shifts, vals


def test_get_2dt_batch_edges(gpu):
    shifts, vals = _2dt_inputs()
    lay = (5, 3, 1, 2, 30, 40, 32)
    gl, ol, gcam, ocam = G.Layout(*lay), O.GeomLayout(*lay), G.Camera(*GC.CAM), O.GeomCamera(*GC.CAM)
    want = []
    for k in range(len(shifts)):
        st, tran, diff = G.get_2dt(shifts[k], gl, gcam, G.T2dParams(*vals[k]))
        wst, wtran, wdiff = O.geom_get_2dt(shifts[k], ol, ocam, O.Geom2dtParams(*vals[k]))
        assert st == wst and np.array_equal(tran, wtran) and np.array_equal(diff, wdiff)     # test_geometry.py: exact on one host
        want.append((wst, wtran, wdiff))
    assert [w[0] for w in want[:8]] == [0, 0, 0, 0, 0, 0, 2, 0] and [want[k][0] for k in (9, 62, 63, 64)] == [1, 2, 1, 1]
    d_sh, d_val = torch.from_numpy(shifts).to(gpu), torch.from_numpy(vals).to(gpu)
    s = torch.cuda.current_stream(gpu)
    for n in (1, 63, 64, 65):                                  # one lane; a ragged block; a full one; a second block of one lane
        out = torch.full((n + GUARD, 8), SENTINEL, dtype=torch.float64, device=gpu)
        _capi.check(_capi.load().mof_geom_get_2dt_batch_device(d_sh.data_ptr(), C.byref(gl), C.byref(gcam), d_val.data_ptr(), n,
                                                               out.data_ptr(), C.c_void_p(s.cuda_stream)))
        wrapped = G.get_2dt_batch_device(d_sh[:n].contiguous(), gl, gcam, d_val[:n].contiguous())
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:n].view(np.int64), wrapped.cpu().numpy().view(np.int64))
        assert (got[n:].view(np.int64) == np.float64(SENTINEL).view(np.int64)).all(), (n, got[n:])
        assert not np.isnan(got).any()
        for k in range(n):
            wst, wtran, wdiff = want[k]
            assert got[k, 6] == wst and got[k, 7] == 0.0, (n, k, got[k], wst)
            assert np.allclose(got[k, :3], wtran, rtol=1e-12, atol=1e-12) and np.allclose(got[k, 3:6], wdiff, rtol=1e-9, atol=1e-11), (k, got[k])
            if wst != 0:
                assert not got[k, :6].any()
