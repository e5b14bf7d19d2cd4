"""Host side of the block matchers' quality outputs and match gate; no GPU.

 1. the inputs of test_gpu_bm_quality.py are what they claim to be, shown on the CPU oracle: the directed pairs put the unique arg-max of
    every block at each corner of the shift square, the scenes leave a gap on both measures with blocks on either side, the 120-pixel
    block's sums pass 2^16 and the 16-pixel scans' reach the top bit of a 16-bit field;
 2. the ABI: argument checks of the new entries on a box without a device, MOF_BM_INVALID against radius <= 48;
 3. the LDS arithmetic of the scans' quality form for every supported (block, radius): never beyond 160 KB, the plain plan unchanged by it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bm_quality_cases as BQ
from mrs_optic_flow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_MAX = 160 * 1024


# ---- 1. the cases ----
@pytest.mark.parametrize("name", list(BQ.SHAPES))
def test_directed_pairs_put_the_maximum_at_each_corner(name):
    b = BQ.batch(name, "directed")
    d = 2 * b.shape.radius
    for k, (cx, cy) in enumerate(BQ.CORNERS):
        for p in range(b.shape.blocks):
            sad = b.sad[k, p]
            assert sad[cy * d, cx * d] == sad.max() and int((sad == sad.max()).sum()) == 1, (name, k, p)
    # xs = 2r is scan16's v_sad_u8 column; in the generic scan it lies in the last group of four x-shifts, padded here (D % 4 != 0)
    assert any(cx for cx, _ in BQ.CORNERS) and (b.shape.scan16 or (d + 1) % 4 != 0)


@pytest.mark.parametrize("name", list(BQ.SHAPES))
def test_scenes_leave_a_gap_on_both_measures(name):
    b = BQ.batch(name, "scenes")
    a, r, (m_lo, m_hi, r_lo, r_hi) = b.thresholds()
    px = b.shape.block ** 2
    print(f"{name}: min_sad matched <= {m_lo / px:.1f}/px, unrelated >= {m_hi / px:.1f}/px; range unrelated <= {r_lo / px:.1f}/px, matched >= {r_hi / px:.1f}/px")
    assert m_lo < a < m_hi and r_lo < r <= r_hi, (name, m_lo, m_hi, r_lo, r_hi)
    for thr in ((a, 0), (0xFFFFFFFF, r), (a, r)):
        v = b.valid(*thr)
        assert v[0].all() and not v[1].any(), (name, thr)
        assert v.any() and not v.all()
    if b.shape.blocks > 1:  # the mixed pair has blocks on either side under both measures together
        v = b.valid(a, r)[2]
        assert v.any() and not v.all(), name


def test_large_sums_and_top_bits():
    assert BQ.batch("g120-r21", "hard").quality[..., 2].max() > 1 << 16
    for name in ("s16-r2", "s16-r6", "s16-r8", "s16-r16"):
        assert BQ.batch(name, "hard").quality[..., 2].max() >= 1 << 15, name  # an unsigned compare or nothing
    cur, prev = BQ.constant_block_method()
    assert (cur == prev).all()


# ---- 2. the ABI ----
def test_invalid_constant_lies_outside_every_scan_range():
    src = open(os.path.join(ROOT, "include", "mof.h")).read()
    m = re.search(r"#define MOF_BM_INVALID \((-?\d+)\)", src)
    assert m and int(m.group(1)) == _capi.MOF_BM_INVALID == BQ.INVALID == -128
    assert np.int8(_capi.MOF_BM_INVALID) == -128  # representable in the outputs' type
    lib, out = _capi.load(), (C.c_int * 4)()
    assert lib.mof_bm_scan_plan(16, 0, 48, 0, 0, out) == _capi.MOF_OK      # the largest radius the kernels take ...
    assert lib.mof_bm_scan_plan(16, 0, 49, 0, 0, out) == _capi.MOF_ERR_BAD_ARG  # ... and the first they refuse
    assert _capi.MOF_BM_INVALID < -48


def test_new_entries_check_their_arguments_without_a_device():
    lib = _capi.load()
    a, b = C.c_uint32(1), C.c_uint32(2)
    n = C.c_int(0)
    assert lib.mof_bm_set_gate(None, 1, 2) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_bm_gate(None, C.byref(a), C.byref(b)) == _capi.MOF_ERR_NOT_INIT and (a.value, b.value) == (1, 2)
    assert lib.mof_shard_bm_set_gate(None, 1, 2) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_shard_bm_gate(None, C.byref(a), C.byref(b)) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_bm_process_q(None, None, 0, None, None, None, None, C.byref(n)) == _capi.MOF_ERR_NOT_INIT
    for fn in (lib.mof_bm_process_batch_device_q, lib.mof_bm_process_batch_device_bgr_q):
        assert fn(None, None, 0, None, 0, 0, 1, None, None, None, None, None, None) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_bm_process_batch_host_q(None, None, 0, None, 0, 0, 1, None, None, None, None, None) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_bm_scan_plan(16, 0, 8, 4, 1, None) == _capi.MOF_ERR_BAD_ARG
    assert lib.mof_bm_scan_plan(18, 0, 8, 4, 1, (C.c_int * 4)()) == _capi.MOF_ERR_BAD_ARG  # block not a multiple of 4
    assert b"mof_bm_scan_plan" in lib.mof_last_error()


# ---- 3. the plan of the quality form ----
def _plan(lib, block, step, radius, grid_x, q):
    out = (C.c_int * 4)()
    rc = lib.mof_bm_scan_plan(block, step, radius, grid_x, q, out)
    return None if rc != _capi.MOF_OK else tuple(out)


def test_quality_plan_lds_for_every_supported_geometry():
    """Every supported (block, radius) at grid_x = 0 (any), 1, 2, 3, 5, 16, 40: the quality form's LDS never passes 160 KB; it is the plain
    plan plus 4 bytes per block slot (generic scan) or plus one 64-entry array (scan16), on the same blocks per workgroup -- or on one
    fewer where the extra bytes would not fit, which no geometry of this sweep needs; the plain plan is what it is without the quality form
    (asked for before and after)."""
    lib = _capi.load()
    supported = smaller = 0
    for block in range(4, 129, 4):
        for radius in range(1, 49):
            if _plan(lib, block, 0, radius, 0, 0) is None:
                continue
            supported += 1
            for grid_x in (0, 1, 2, 3, 5, 16, 40):
                for step in ((0, 8) if block == 16 else (0,)):
                    plain = _plan(lib, block, step, radius, grid_x, 0)
                    q = _plan(lib, block, step, radius, grid_x, 1)
                    assert plain == _plan(lib, block, step, radius, grid_x, 0)
                    assert q[0] == plain[0] and q[3] <= LDS_MAX and plain[3] <= LDS_MAX, (block, radius, grid_x, plain, q)
                    if plain[0]:  # scan16: one wave, 64 KB of LDS at the most
                        assert q[1:3] == plain[1:3] and q[3] == plain[3] + 256 and q[3] <= 64 * 1024
                    elif q[1] == plain[1]:
                        assert q[2] == plain[2] and q[3] == plain[3] + 4 * plain[1]
                    else:
                        smaller += 1
                        assert q[1] == plain[1] - 1 and plain[3] + 4 * plain[1] > LDS_MAX and q[2] <= plain[2]
    assert supported > 1000 and smaller == 0, (supported, smaller)


_LDS_FULL_SCRIPT = """
import ctypes as C, sys
sys.path.insert(0, {root!r})
from mrs_optic_flow_amd import _capi
lib = _capi.load()
LDS_MAX = 160 * 1024
def _plan(block, step, radius, grid_x, q):
    out = (C.c_int * 4)()
    rc = lib.mof_bm_scan_plan(block, step, radius, grid_x, q, out)
    return None if rc != _capi.MOF_OK else tuple(out)
for grid_x in (7, 13, 14, 28):
    plain, q = _plan(100, 0, 4, grid_x, 0), _plan(100, 0, 4, grid_x, 1)
    assert plain == (0, 7, 128, 163828) and plain[3] + 4 * plain[1] > LDS_MAX, plain
    assert q[0] == 0 and q[1] == 6 and q[2] == 128 and q[3] == (163828 - 12 * 7) // 7 * 6 + 16 * 6 <= LDS_MAX, q
print("lds full ok")
"""


def test_quality_plan_takes_one_block_fewer_where_the_lds_is_full():
    """The one plan family that reaches the limit (found by sweeping grid_x = 0 .. 64 under MOF_BM_XB = 1, 2, 3): block 100, radius 4 with two
    groups of x-shifts per lane holds 7 blocks in 163 828 bytes; 28 more would pass 163 840, so the quality form launches 6. The knob is read
    once per process, so the four geometries are asked in a child process that starts with it set."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-c", _LDS_FULL_SCRIPT.format(root=ROOT)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, MOF_BM_XB="2"))
    assert r.returncode == 0 and "lds full ok" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
