"""CPU half of the geometry-tail path tests: every case of geom_cases.py through the library's host form and through the oracle
(oracle/geom_ref.c) by test_geometry.py's rule -- status and inlier mask equal, rot / tran / H to 1e-9, planted scenes recover the planted
consensus set -- and then the proof that the cases reach the device paths they were built for, so that test_gpu_geometry_paths.py cannot
pass by missing them. The scan is replayed by tests/cpp/geom_ransac_probe.cpp (geom_core.hpp's own ransac_hypothesis / ransac_accept).

Measured here (x86-64, glibc; 32 pairs per late geometry):
  late, pairs accepted at best_iter >= 64 (exact / noisy): 13x5 11 / 18, 5x13 9 / 22, 16x16 16 / 24, 17x15 14 / 23, 32x32 12 / 22,
    20x13 13 / 21; the same pairs change their best model in two or more rounds; the latest accepted hypothesis is 1363 (20x13 noisy)
  late, final niters: 239 / 427 / 955 (65 patches) ... 249 / 473 / 1200 (1024) by share of invalid patches: every one ends inside a round
  late valid counts: 55 / 60 / 65, 214 / 235 / 256, 213 / 234 / 255, 217 / 239 / 260, 854 / 939 / 1024
  fit_forms: 4 (exact) and 6 (noisy) of 8 low-inlier pairs accept beyond the first round, none of the 90 % ones (index <= 7)
  exits: 257x1 accepts at 8, 19, 83, 14; no consensus 32x32 scans all 2000
  statuses: late, fit_forms {0}; small_n {0, 2, 3, 8}; exits {0, 1, 2, 3, 4, 5, 6, 7, 8}
  host form against oracle over all 493 cases: status and mask equal, rot / tran / H differ by at most 2.8e-17"""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import geom_cases as GC

_probe = None


def scan(case):
    """-> (best_iter, final niters, changes of the best model, rounds of 64 in which it changed) of the case's RANSAC scan"""
    global _probe
    if _probe is None:
        here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
        if not os.path.exists(os.path.join(here, "geom_ransac_probe.so")):
            subprocess.check_call(["make", "-C", here, "-s", "geom_ransac_probe.so"])
        _probe = C.CDLL(os.path.join(here, "geom_ransac_probe.so"))
        _probe.geom_ransac_probe.restype = None
        _probe.geom_ransac_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    a, b = case.points()
    out = (C.c_int * 4)()
    _probe.geom_ransac_probe(a.ctypes.data, b.ctypes.data, len(a), out)
    return tuple(out)


FAMILIES = {"late": GC.late, "small_n": GC.small_n, "exits": GC.exits, "fit_forms": lambda: GC.fit_forms()[0] + GC.fit_forms()[1]}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_host_form_equals_oracle_on_every_case(family):
    refs = GC.references()
    worst = 0.0
    statuses = collections.Counter()
    for c in FAMILIES[family]():
        (st, rot, tran, mask, H), (wst, wrot, wtran, wmask, wH) = refs[c.name]
        assert st == wst and np.array_equal(mask, wmask), (c.name, st, wst)
        for got, want in ((rot, wrot), (tran, wtran), (H, wH)):
            assert np.allclose(got, want, rtol=0, atol=1e-9), (c.name, got, want)
            worst = max(worst, float(np.abs(got - want).max()))
        if st != 0:
            assert np.array_equal(rot, [0, 0, 0, 1]) and not tran.any(), (c.name, rot, tran)
        elif c.planted is not None:
            assert np.array_equal(mask.astype(bool), c.planted), (c.name, np.flatnonzero(mask.astype(bool) != c.planted))
        statuses[st] += 1
    print(f"\n{family}: {sum(statuses.values())} cases, statuses {dict(sorted(statuses.items()))}, host - oracle <= {worst:.3g}")


def test_late_scenes_reach_the_later_rounds():
    groups = collections.OrderedDict()
    for c in GC.late():
        groups.setdefault(c.group, []).append(scan(c))
    assert len(groups) == 2 * len(GC.LATE_GRIDS)
    for name, scans in groups.items():
        late = sum(best >= 64 for best, _, _, _ in scans)
        cut = [n for _, n, _, _ in scans if n > 64 and n % 64]
        two = sum(rounds >= 2 for _, _, _, rounds in scans)
        print(f"\n{name}: {late} of {len(scans)} accept at best_iter >= 64 (latest {max(s[0] for s in scans)}), {len(cut)} end inside a later "
              f"round (niters {sorted(set(cut))}), {two} change their best model in two or more rounds")
        assert len(scans) == GC.PAIRS and 4 * late >= len(scans), (name, late)   # `owner = best_iter - base` with base > 0, checked by value
        assert cut, name                                                         # `base < scan.niters` between rounds, the cut inside one
        assert two >= 1, name                                                    # best[] overwritten by a later round's shuffle
    # the scan is the host form's: a pair that ends in status 0 has a best model
    assert all(best >= 0 for scans in groups.values() for best, _, _, _ in scans)


def test_fit_form_pairs_hold_the_same_points():
    """the premise of the device's bit-equality test: both layouts give the tail the same a, b and n, and the host form the same bits"""
    refs = GC.references()
    small, padded = GC.fit_forms()
    assert len(small) == len(padded) == 4 * GC.FIT_PAIRS
    late = 0
    for c, d in zip(small, padded):
        assert c.total == 256 and d.total == 272 and not d.valid[256:].any()
        (a, b), (a2, b2) = c.points(), d.points()
        assert np.array_equal(a, a2) and np.array_equal(b, b2)
        h, h2 = refs[c.name][0], refs[d.name][0]
        assert h[0] == h2[0] == 0 and np.array_equal(h[1], h2[1]) and np.array_equal(h[2], h2[2]) and np.array_equal(h[4], h2[4])
        assert np.array_equal(h[3], h2[3][:256])
        late += scan(c)[0] >= 64
    print(f"\nfit_forms: {late} of {len(small)} pairs accept at best_iter >= 64")
    assert late >= 4


def test_cases_cover_every_status_and_the_edge_counts():
    refs = GC.references()
    statuses, valid = set(), set()
    for c in GC.everything():
        statuses.add(refs[c.name][0][0])
        valid.add(int(c.valid.sum()))
    print(f"\nstatuses {sorted(statuses)}; valid counts {sorted(valid)}")
    assert statuses == {0, 1, 2, 3, 4, 5, 6, 7, 8}
    assert {0, 3, 4, 5, 6, 7, 63, 64, 65, 256, 257, 1024} <= valid
    totals = {c.total for c in GC.everything()}
    assert {65, 255, 256, 257, 260, 272, 1024} <= totals                         # 64 + 1, 4 * 64 - 1, kWaveFitPoints and + 1, 4 * 64 + 4, kMaxPoints
    assert any(c.layout[0] > c.layout[1] for c in GC.late()) and any(c.layout[0] < c.layout[1] for c in GC.late())
    # few valid points on the 7 x 5 grid: (valid, thr) -> status
    want = {(0, 0): 8, (3, 0): 8, (3, 3): 3, (4, 4): 0, (4, 0): 0, (5, 4): 0, (5, 5): 0, (4, 5): 2}
    seen = {(int(c.valid.sum()), c.thr): refs[c.name][0][0] for c in GC.small_n() if c.total == 35}
    assert all(seen[k] == v for k, v in want.items()), seen
    by_name = {c.name: refs[c.name][0] for c in GC.exits()}
    assert by_name["exits pure rotation"][0] == 0 and by_name["exits pure rotation, NaN IMU"][0] == 5
    assert by_name["exits pure rotation, height inf"][0] == 6 and by_name["exits general motion, NaN IMU"][0] == 7
    hover = by_name["exits zero shifts (hover)"]
    assert hover[0] == 0 and np.allclose(hover[1], [0, 0, 0, 1], rtol=0, atol=1e-9) and np.allclose(hover[2], 0, rtol=0, atol=1e-12)
    assert [by_name[f"exits dt {n}"][0] for n in ("0", "-0", "NaN")] == [1, 1, 1]
    assert by_name["exits thr -1"][0] == 2 and by_name["exits all NaN"][0] == 2 and by_name["exits no consensus 32x32"][0] == 3
    for g in ("12x1", "1x12"):
        assert [by_name[f"exits collinear {g} {cam} thr {t}"][0] for cam in ("flat", "distorted") for t in (0, 8)] == [8, 3, 0, 0]
