"""The kernels against the RECORDED outputs of the reference's own OpenCL text (tests/golden/ref_cl_bm.npz, ref_cl_fft_peak.npz;
written by tests/golden/make_ref_cl_fixtures.py from the text executed on the CPU). Reads only tests/golden/.

Block matching: dx, dy and the top three per axis of FastSpacedBMMethod.process_batch_device, bit-equal to the text's, on both
scans (the register-resident 16 x 16 scan at three radii; the generic scan with eight blocks per workgroup, a ragged row tail,
flushed packed sums). The one-block case holds the documented repair of the text's unsorted Y list.

Peak model: FftMethod(peak_model=PEAK_OCL) on the recorded patch pairs within tolerances.TOL of the text's result. Each pair is a
frame of its own, i.e. patch (0, 0), the placement the result was recorded at: there the text's float sums over absolute
coordinates stay within about 1e-5 px of the exact centroid of the same surface (at the far patch of a 7 x 7 field of 120-pixel
patches they drift by up to 1.5e-4 px, which tests/test_ref_cl_host.py holds bit for bit against the f32 oracle instead)."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import FastSpacedBMMethod, FftMethod
from tolerances import TOL

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def bm_fixture():
    with np.load(os.path.join(GOLDEN, "ref_cl_bm.npz")) as g:
        return {k: g[k] for k in g.files}


def _bm_names():
    with np.load(os.path.join(GOLDEN, "ref_cl_bm.npz")) as g:
        return [str(s) for s in g["names"]]


@pytest.mark.parametrize("k,name", list(enumerate(_bm_names())))
def test_block_matching_equals_the_reference_text(gpu, bm_fixture, k, name):
    g = bm_fixture
    block, step, radius, _ = (int(v) for v in g["params"][k])
    cur, prev = g[f"cur{k}"], g[f"prev{k}"]
    h, w = cur.shape
    assert h <= 200 and w <= 330
    eng = FastSpacedBMMethod(block, radius, step, (h, w))
    dx, dy, mode = eng.process_batch_device(torch.from_numpy(cur[None]).to(gpu), torch.from_numpy(prev[None]).to(gpu))
    dx, dy, mode = dx.cpu().numpy()[0], dy.cpu().numpy()[0], mode.cpu().numpy()[0]
    assert np.array_equal(dx, g[f"dx{k}"]) and np.array_equal(dy, g[f"dy{k}"]), name
    top_x, top_y = mode[0:6:2], mode[1:6:2]
    assert np.array_equal(top_x, g["top_x"][k]), (name, top_x, g["top_x"][k])
    if dx.size == 1:
        # the known reference defect: the text leaves Y unsorted on a one-block grid; the
        # kernels return the sorted list
        repaired = [int(dy[0, 0])] + [v for v in range(-radius, radius + 1) if v != dy[0, 0]][:2]
        assert top_y.tolist() == repaired and g["top_y"][k].tolist() != repaired, (name, top_y, g["top_y"][k])
        assert g["top_y"][k].tolist() == [-radius, -radius + 1, -radius + 2]
    else:
        assert np.array_equal(top_y, g["top_y"][k]), (name, top_y, g["top_y"][k])


def test_block_matching_fixture_covers_both_scans():
    names = _bm_names()
    for must in ("gpu-scan16-r2", "gpu-scan16-r8", "gpu-scan16-r16", "gpu-generic-8-blocks-per-group", "gpu-generic-ragged-row",
                 "gpu-generic-flushed-sums", "one-block-r4", "low-contrast-r5"):
        assert must in names, must


@pytest.mark.parametrize("n", [32, 64, 120])
def test_ocl_peak_model_within_tol_of_the_reference_text(gpu, n):
    from mrs_optic_flow_amd.engine import PEAK_OCL
    with np.load(os.path.join(GOLDEN, "ref_cl_fft_peak.npz")) as g:
        cur, prev, want, ok_rec = g[f"cur{n}"], g[f"prev{n}"], g[f"pair_ref{n}"][:, 0], g[f"pair_ok{n}"]
    fm = FftMethod(sample_point_size=n, frame_shape=(n, n), grid=(1, 1), origin=(0, 0), stride=(n, n), peak_model=PEAK_OCL)
    got = fm.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)).cpu().numpy()[:, 0]
    used = 0
    for k in range(cur.shape[0]):
        _, d = O.phase_correlate_ocl(cur[k], prev[k], (0, 0), 55, 32)
        ok = bool(np.isfinite(d["peak_value"]) and d["second_value"] < 0.5 * d["peak_value"])  # the suite's usual filter
        assert ok == bool(ok_rec[k])
        err = np.abs(got[k] - want[k].astype(np.float64)).max()
        print(f"n {n} pair {k}: kernel {got[k].tolist()} text {want[k].tolist()} |diff| {err:.2e} {'' if ok else '(filtered out)'}")
        if ok:
            assert err <= TOL, (n, k, got[k], want[k])
            used += 1
    assert used >= 0.8 * cur.shape[0]
