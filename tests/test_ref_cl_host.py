"""The oracle against the reference's OWN OpenCL text, executed on the CPU (oracle/cl_host.h; oracle/_ref/libref_bm_cl.so and
libref_fft_peak_{32,64,120}.so, which build() makes where the reference checkout exists).

Block matching: OptFlow_C1_D0 + Histogram_C1_D0 against oracle_bm_process_u8 / oracle_bm_histogram_top -- per-block shifts and the
top three per axis, bit-exact. Peak stage: minmaxloc + refine against oracle_ocl_peak_f32 on the same f32 surface -- bit equality
of the two float results (both do the same float operations in the same order, both built without contraction).

One known divergence, a reference defect that the project repairs (note F13): on a 1 x 1 grid the text
never sorts its Y histogram. test_one_block_grid_known_reference_defect holds both behaviours side by side; no other divergence
was found.

Without the libraries AND without the checkout these tests skip (there is nothing to run); with the checkout, missing libraries
fail. The recorded outputs of tests/golden/ref_cl_*.npz hold the oracle everywhere (test_recorded_* need no library)."""
import os

import numpy as np
import pytest

import oracle_lib as O
import ref_cl as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def ref():
    if not R.usable():
        if R.reference_checkout_present():
            pytest.fail(f"the reference checkout is present but {R.REF_OUT} lacks a library: build() (make -C oracle ref) must make them")
        pytest.skip("no reference checkout and no oracle/_ref libraries: the reference's text cannot be executed here")
    return R


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _check_bm(c, ref):
    rdx, rdy, rtx, rty = ref.bm_reference(c)
    odx, ody, otx, oty = ref.bm_oracle(c)
    bad = []
    if not (np.array_equal(rdx, odx) and np.array_equal(rdy, ody)):
        bad.append(f"{c.name}: shifts differ: text dx {rdx.tolist()} dy {rdy.tolist()}, oracle dx {odx.tolist()} dy {ody.tolist()}")
    if not (np.array_equal(rtx, otx) and np.array_equal(rty, oty)):
        bad.append(f"{c.name}: top-3 differ: text x {rtx.tolist()} y {rty.tolist()}, oracle x {otx.tolist()} y {oty.tolist()}")
    return bad


def test_peak_libraries_carry_the_hosts_defines(ref):
    """kercn, WGS and WGS2_ALIGNED each peak library was compiled with are the ones the reference's host derives for its n."""
    for n in R.PEAK_SIZES:
        got = np.zeros(4, np.int32)
        ref.peak_lib(n).ref_fft_peak_params(got.ctypes.data)
        kercn, wgs, w2 = R.peak_params(n)
        assert tuple(got) == (n, kercn, wgs, w2), (n, got)
        assert wgs > w2, "every size exercises the lid >= WGS2_ALIGNED merge"
    assert R.peak_params(120) == (8, 15, 8) and R.peak_params(32) == (8, 4, 2) and R.peak_params(64) == (8, 8, 4)


def test_block_matching_sweep(ref):
    cases = R.bm_sweep_cases()
    assert len(cases) >= 150 and all(c.grid[0] * c.grid[1] >= 2 for c in cases)
    assert {c.scan_block == 2 * c.radius + 1 for c in cases} == {True, False}
    bad = [m for c in cases for m in _check_bm(c, ref)]
    print(f"block-matching sweep: {len(cases)} cases, {len(bad)} divergences")
    assert not bad, "\n".join(bad)


def test_block_matching_engineered(ref):
    cases = R.bm_engineered_cases() + R.bm_gpu_cases()
    bad = [m for c in cases for m in _check_bm(c, ref)]
    print(f"block-matching engineered: {len(cases)} cases, {len(bad)} divergences")
    assert not bad, "\n".join(bad)


def test_block_matching_known_answers(ref):
    """What the engineered cases are FOR, asserted on the text's output (the oracle equals it by the test above)."""
    by = {c.name: c for c in R.bm_engineered_cases()}
    for name, c in by.items():
        if name.startswith(("constant-", "saturated-const-")):  # every SAD ties; centre - min = 0 <= 0.2 r^2 -> (0, 0)
            dx, dy, tx, ty = ref.bm_reference(c)
            assert not dx.any() and not dy.any()
            assert tx.tolist() == [0, -c.radius, -c.radius + 1] and ty.tolist() == tx.tolist()  # empty bins stay in index order
    dx, dy, _, _ = ref.bm_reference(by["low-contrast-r5"])
    assert (dx[0, 0], dy[0, 0]) == (0, 0), "gap 5 == 0.2 * 25: zeroed"
    assert (dx[0, 1], dy[0, 1]) == (1, -5), "gap 6: kept -- the first candidate in row-major order that misses the raised pixel"
    _, _, tx, ty = ref.bm_reference(by["hist-ties-3-bins"])
    assert tx.tolist() == [-1, 2, 3] and ty.tolist() == [-4, 0, 4]  # equal counts: ascending shift
    _, _, tx, ty = ref.bm_reference(by["hist-ties-and-singles"])
    assert tx.tolist() == [-1, 2, 3] and ty.tolist() == [-2, 1, 0]
    _, _, tx, ty = ref.bm_reference(by["hist-one-bin"])
    assert tx.tolist() == [1, -4, -3] and ty.tolist() == [-4, -3, -2]
    _, _, tx, ty = ref.bm_reference(by["hist-two-bins"])
    assert tx.tolist() == [4, -4, -3] and ty.tolist() == [2, -3, -4]
    _, _, tx, ty = ref.bm_reference(by["hist-two-bins-tied"])
    assert tx.tolist() == [-2, 3, -4] and ty.tolist() == [-4, 4, -3]
    _, _, tx, ty = ref.bm_reference(by["hist-all-distinct"])
    assert tx.tolist() == [-4, -3, -2] and ty.tolist() == [-4, -3, -2]
    for name in ("periodic-b8r6", "periodic-b16r9", "periodic-b4r12"):
        c = by[name]
        dx, dy, _, _ = ref.bm_reference(c)
        _, _, _, sad = O.bm_process(c.cur, c.prev, O.bm_config_fast_spaced(c.cur.shape[1], c.cur.shape[0], c.block, c.step, c.radius), want_sad=True)
        assert ((sad.reshape(sad.shape[0], -1) == 0).sum(axis=1) > 1).all(), "several exact minima per block"
        first = np.array([divmod(int(np.argmin(s)), 2 * c.radius + 1) for s in sad]) - c.radius
        assert np.array_equal(dy.ravel(), first[:, 0]) and np.array_equal(dx.ravel(), first[:, 1])


def test_one_block_grid_known_reference_defect(ref):
    """Histogram_C1_D0 sorts X in work-item 0 and Y in work-item 1 (.cl:127-151); a 1 x 1 grid launches one work-item, so the Y
    list comes back unsorted: (-r, -r+1, -r+2) whatever the block found. The oracle and every kernel return the sorted list (the
    evident intent). Both are asserted here, side by side, so that neither can change unnoticed."""
    for c in R.bm_one_block_cases():
        sx, sy = c.true_shift
        r = c.radius
        rdx, rdy, rtx, rty = ref.bm_reference(c)
        odx, ody, otx, oty = ref.bm_oracle(c)
        assert rdx.tolist() == [[sx]] and rdy.tolist() == [[sy]] and np.array_equal(odx, rdx) and np.array_equal(ody, rdy)
        rest = [v for v in range(-r, r + 1) if v != sx][:2]
        assert rtx.tolist() == [sx] + rest and np.array_equal(otx, rtx)                # X: sorted in both
        assert rty.tolist() == [-r, -r + 1, -r + 2]                                    # Y, the text: never sorted
        assert oty.tolist() == [sy] + [v for v in range(-r, r + 1) if v != sy][:2]     # Y, the oracle: the repaired answer
        assert (rty.tolist() != oty.tolist()) == (sy != -r)
    print("block matching: the 1 x 1 grid's unsorted Y list is the only divergence between the reference text and the oracle")


@pytest.mark.parametrize("n", R.PEAK_SIZES)
def test_peak_stage_bit_equal(ref, n):
    cases = R.peak_cases(n)
    names = [c[0] for c in cases]
    for must in ("pair0", "peak-y0-x0", f"peak-y{n - 1}-x{n - 2}", "row-tie-same-item", "three-way-tie", "all-negative", "all-zero",
                 f"lid{R.peak_params(n)[1] - 1}"):
        assert must in names, must
    assert any(s.startswith("row-tie-lid0-lid") for s in names) and any(s.startswith("cross-row-tie") for s in names)
    frame = np.full((R.FIELD * n, R.FIELD * n), 1000.0, np.float32)
    bad = []
    for name, surf, _ in cases:
        for xv, yv in R.PEAK_ORIGINS:
            want = ref.peak_reference(surf, xv, yv, frame)
            got = R.peak_oracle(surf, xv, yv)
            if not np.array_equal(_bits(want), _bits(got)):
                bad.append(f"n {n} {name} at patch ({xv}, {yv}): text {want.tolist()} oracle {got.tolist()}")
    print(f"peak stage n {n}: {len(cases)} surfaces x {len(R.PEAK_ORIGINS)} origins, {len(bad)} not bit-equal")
    assert not bad, "\n".join(bad[:20])


@pytest.mark.parametrize("n", R.PEAK_SIZES)
def test_peak_stage_known_answers(ref, n):
    """What the synthetic surfaces are FOR, asserted on the text's output."""
    by = dict(R.synthetic_surfaces(n))
    h = n // 2
    kercn, wgs, w2 = R.peak_params(n)
    for name in ("all-negative", "max-is-zero", "all-zero", "one-tiny-positive"):
        # nothing (or nothing that survives FLT_EPSILON) positive: centroid 0, result -(origin + n/2); at the far origin too
        for xv, yv in R.PEAK_ORIGINS:
            got = ref.peak_reference(by[name], xv, yv)
            if name == "one-tiny-positive":  # x * 1e-30 / FLT_EPSILON: the centroid is of the order 1e-21, lost against n/2
                assert got.tolist() == [-(xv * n + h), -(yv * n + h)]
            else:
                assert got.tolist() == [-float(xv * n + h), -float(yv * n + h)], (name, got)
    # a tie: the answer is the centroid around the FIRST member in row-major order, i.e. equal to the surface without the others
    for name, s in by.items():
        if name.startswith("cross-row-tie"):
            ya, xa, yb, xb = (int(v) for v in name.split("-")[3:])
            alone = s.copy()
            alone[max(0, yb - 3):yb + 4, max(0, xb - 3):xb + 4] = np.float32(-1.0)
            assert np.array_equal(_bits(ref.peak_reference(s, 0, 0)), _bits(ref.peak_reference(alone, 0, 0))), name
            got = ref.peak_reference(s, 0, 0)
            assert abs(got[0] + h - xa) < 1.5 and abs(got[1] + h - ya) < 1.5, (name, got)
        if name.startswith("row-tie-lid"):
            la = int(name.split("-")[2][3:])
            got = ref.peak_reference(s, 0, 0)
            assert abs(got[0] + h - (la * kercn + 1)) < 1.5, (name, got)
    for lid in range(w2, wgs):  # a maximum only a work-item >= WGS2_ALIGNED holds is found
        s = by[f"lid{lid}"]
        y, x = np.unravel_index(int(np.argmax(s)), s.shape)
        assert x // kercn == lid
        got = ref.peak_reference(s, 0, 0)
        assert abs(got[0] + h - x) < 1.5 and abs(got[1] + h - y) < 1.5, (lid, got)
    # clamped windows hold 4 .. 7 cells per axis: a constant surface's centroid is the window's centre
    got = ref.peak_reference(by["constant-positive"], 0, 0)
    assert np.allclose(got, [1.5 - h, 1.5 - h], atol=1e-5)


def test_pairs_pass_the_usual_filter():
    """At least 80 % of the recorded patch pairs pass the suite's second-peak filter (the GPU test uses only those)."""
    for n in R.PEAK_SIZES:
        ok = [d["second_value"] < 0.5 * d["peak_value"] for d in (R.pair_surface(c, p)[1] for c, p in R.patch_pairs(n))]
        assert sum(ok) >= 0.8 * len(ok) and len(ok) >= 10, (n, ok)
        assert not all(ok), "one pair is unrelated noise on purpose: the filter must be seen to reject"


# ---- the recorded fixtures -----------------------------------------------------------------------------------------------

def test_fixtures_reproduce(ref):
    """tests/golden/ref_cl_*.npz regenerated in memory from the reference text: every array equal to the committed one."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ref_cl_fixtures", os.path.join(GOLDEN, "make_ref_cl_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for fname, fresh in (("ref_cl_bm.npz", mod.bm_arrays()), ("ref_cl_fft_peak.npz", mod.fft_peak_arrays())):
        with np.load(os.path.join(GOLDEN, fname)) as g:
            assert sorted(g.files) == sorted(fresh), fname
            for k in g.files:
                a, b = g[k], np.asarray(fresh[k])
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (fname, k)


def test_recorded_block_matching_holds_the_oracle():
    """No library needed: the oracle against the reference text's RECORDED outputs."""
    with np.load(os.path.join(GOLDEN, "ref_cl_bm.npz")) as g:
        names = [str(s) for s in g["names"]]
        assert len(names) >= 25
        for k, name in enumerate(names):
            block, step, radius, scan_block = (int(v) for v in g["params"][k])
            c = R.BmCase(name, g[f"cur{k}"], g[f"prev{k}"], block, step, radius, scan_block)
            odx, ody, otx, oty = R.bm_oracle(c)
            assert np.array_equal(odx, g[f"dx{k}"]) and np.array_equal(ody, g[f"dy{k}"]), name
            assert np.array_equal(otx, g["top_x"][k]), name
            if c.grid == (1, 1):  # the known reference defect: recorded as the text gives it, repaired by the oracle
                assert g["top_y"][k].tolist() == [-radius, -radius + 1, -radius + 2] and oty[0] == ody[0, 0] != -radius, name
            else:
                assert np.array_equal(oty, g["top_y"][k]), name


def test_recorded_peak_stage_holds_the_oracle():
    with np.load(os.path.join(GOLDEN, "ref_cl_fft_peak.npz")) as g:
        for n in R.PEAK_SIZES:
            cur, prev, want = g[f"cur{n}"], g[f"prev{n}"], g[f"pair_ref{n}"]
            assert cur.shape[0] >= 10 and want.shape == (cur.shape[0], len(R.PEAK_ORIGINS), 2)
            for k in range(cur.shape[0]):
                surf = R.pair_surface(cur[k], prev[k])[0]
                for j, (xv, yv) in enumerate(R.PEAK_ORIGINS):
                    assert np.array_equal(_bits(R.peak_oracle(surf, xv, yv)), _bits(want[k, j])), (n, k, xv, yv)
        names, surfs, want = [str(s) for s in g["synthetic_names32"]], g["synthetic32"], g["synthetic_ref32"]
        assert len(names) >= 40
        for k, name in enumerate(names):
            for j, (xv, yv) in enumerate(R.PEAK_ORIGINS):
                assert np.array_equal(_bits(R.peak_oracle(surfs[k], xv, yv)), _bits(want[k, j])), (name, xv, yv)
