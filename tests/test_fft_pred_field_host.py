"""No-GPU conditions on the inputs of test_gpu_fft_pred_field.py (tests/pred_field_cases.py): the CPU oracles ALONE must meet them, so that
the GPU test cannot hide behind its inputs. The long-range shifts of the two oracles predict alike and stand off every rounding tie; the
cells of a pair predict differently; each wrong prediction map a kernel could hold -- a transposed index, swapped i and j, a wrong
divisor, a dropped pair offset, a modulo for the clamp -- changes the applied predictions of these scenes (numpy, on the oracle's
long-range shifts: no kernel is mutated); at least half the planted patches are inside patches, each with a clear peak and the two
oracles within the fast path of tests/tolerances.py. Nothing here asserts closeness to a planted shift: the oracle is the reference."""
import numpy as np
import pytest

import pred_cases as PC
import pred_field_cases as FC
import route_cases as R
import tolerances

TIE = 0.48  # |4 s - rint(4 s)| of a long-range component: 0.005 px or more from a rounding tie, fifty times the 1e-4 px bar


def _tie(coarse):
    c = coarse[~np.isnan(coarse)]
    return float(np.abs(4.0 * c - np.rint(4.0 * c)).max())


@pytest.mark.parametrize("l", FC.FIELDS, ids=lambda l: l.name)
def test_layout_is_the_stated_geometry(l):
    gxl, gyl = FC.lr_grid(l)
    assert l.n == 32 and l.origin == (0, 0) and l.stride == (32, 32) and l.pitch >= l.w and l.w % 4 == 0 and l.h % 4 == 0
    assert l.grid[0] * 32 <= l.w and l.grid[1] * 32 <= l.h
    cs = FC.cells(l)
    assert len(cs) == gxl * gyl
    area = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in cs)
    assert area == l.w * l.h and cs[-1][2:] == (l.w, l.h)  # the cells tile the frame, ragged remainder included
    # the cell of a patch by the geometry is the long-range patch of the map
    for p in range(PC.patches(l)):
        i, j = p % l.grid[0], p // l.grid[0]
        assert FC.cell_of(l, p) == min(j // 4, gyl - 1) * gxl + min(i // 4, gxl - 1)
    assert {"f_8x12": (2, 3), "f_11x5": (2, 1), "f_5x11": (1, 2), "f_wide": (2, 1)}[l.name] == (gxl, gyl)


@pytest.mark.parametrize("l", FC.FIELDS, ids=lambda l: l.name)
def test_long_range_oracles_predict_alike_distinctly_and_off_every_tie(l):
    """B.1 - B.3"""
    s = FC.scene(l.name)
    n_lr = len(FC.cells(l))
    assert s.coarse64.shape == (FC.N_PAIRS, n_lr, 2) and not np.isnan(s.coarse64).any()
    for k in range(FC.N_PAIRS):
        preds = [PC.round4_np(*s.coarse64[k, c]) for c in range(n_lr)]
        assert preds == [PC.round4_np(*s.coarse32[k, c]) for c in range(n_lr)], k
        assert len(set(preds)) == n_lr, (k, preds)  # pairwise distinct
        for c, (kind, _, _) in enumerate(s.kinds[k]):
            if kind == "identical":
                assert preds[c] == (0, 0)
            else:
                assert preds[c][0] != 0 and preds[c][1] != 0, (k, c, preds[c])
    assert [k[0] for k in s.kinds[1]].count("identical") == 1 and [k[0] for k in s.kinds[2]].count("constant") == 1
    # planted shifts: multiples of 4, pairwise different inside a pair, a component beyond N / 2, and another assignment in every pair
    for k in range(FC.N_PAIRS):
        planted = [(dx, dy) for kind, dx, dy in s.kinds[k] if kind == "shift"]
        assert len(set(planted)) == len(planted) and all(dx % 4 == 0 and dy % 4 == 0 for dx, dy in planted)
        assert max(max(abs(dx), abs(dy)) for dx, dy in planted) > l.n // 2
    assert len({tuple(s.kinds[k]) for k in range(FC.N_PAIRS)}) == FC.N_PAIRS
    print(f"{l.name}: worst tie margin {_tie(s.coarse64):.3f} (f64), {_tie(s.coarse32):.3f} (f32); bar {TIE}")
    assert _tie(s.coarse64) <= TIE and _tie(s.coarse32) <= TIE


def test_a_constant_cell_has_a_finite_long_range_shift_on_the_reference():
    """What the reference computes for a cell that is constant in both frames, so that nobody expects a NaN there: the flat surface's
    first maximum is bin (0, 0) and its 5 x 5 centroid gives (1 - N / 2, 1 - N / 2) = (-15, -15) quarter-pixels -- finite, inside
    max_px_speed = 80, so the prediction is (-60, -60) before the clamp. The cell whose long-range shift IS NaN beside valid neighbours is
    the gated one (gate_case)."""
    for l in FC.FIELDS:
        s = FC.scene(l.name)
        c = [k[0] for k in s.kinds[2]].index("constant")
        assert np.abs(s.coarse64[2, c] + 15.0).max() < 1e-5 and np.abs(s.coarse32[2, c] + 15.0).max() < 1e-5
        mine = np.array([FC.cell_of(l, p) == c for p in range(PC.patches(l))])
        assert (s.pred[2][mine] == (-60, -60)).all() and not s.inside[2][mine].any()
        # a constant current window answers (1 - N / 2, 1 - N / 2) whatever the previous one shows; the totals of the cell's patches
        # stand clear of the speed gate (80 px) on either side, so the GPU test can state which of them are NaN
        total = s.applied[2][mine] + (1.0 - l.n / 2)
        assert np.abs((total * total).sum(axis=-1) - PC.SPEED ** 2).min() > 40.0


def _mutant(l, coarse, which):
    """the applied predictions under a WRONG map from fine patch (pair k, i, j) to an entry of the coarse array; which = "right" is
    pred_cases.c2f_pred_np's own map"""
    gx, gy = l.grid
    gxl, gyl = gx // 4, gy // 4
    pred = np.zeros((coarse.shape[0], gx * gy, 2), np.int64)
    for k in range(coarse.shape[0]):
        for p in range(gx * gy):
            i, j = p % gx, p // gx
            if which == "swapped":
                i, j = j, i
            d = 2 if which == "divisor" else 4
            if which == "modulo":
                li, lj = (i // d) % gxl, (j // d) % gyl
            else:
                li, lj = min(i // d, gxl - 1), min(j // d, gyl - 1)
            idx = li * gyl + lj if which == "transposed" else lj * gxl + li
            pred[k, p] = PC.round4_np(*coarse[0 if which == "pair0" else k, idx])
    return PC.applied_np(l, pred)


@pytest.mark.parametrize("l", FC.FIELDS, ids=lambda l: l.name)
def test_every_wrong_map_changes_the_applied_predictions(l):
    """B.4: the CPU proof that the scenes would catch those bugs"""
    s = FC.scene(l.name)
    gxl, gyl = FC.lr_grid(l)
    right = _mutant(l, s.coarse64, "right")
    assert np.array_equal(right, s.applied) and np.array_equal(right, PC.applied_np(l, PC.c2f_pred_np(l, s.coarse64)))
    differs = {which: int((_mutant(l, s.coarse64, which) != right).any(axis=-1).sum()) for which in ("transposed", "swapped", "divisor", "pair0", "modulo")}
    print(f"{l.name}: patches whose applied prediction a wrong map changes: {differs}")
    assert differs["swapped"] > 0 and differs["divisor"] > 0 and differs["pair0"] > 0
    if gxl > 1 and gyl > 1:
        assert l.name == "f_8x12" and differs["transposed"] > 0
    else:
        assert differs["transposed"] == 0  # (one row or one column of long-range patches: both orders are the same order)
    # the clamp against a modulo: wherever the GRID is ragged (columns 8 .. 10 of f_11x5, rows 8 .. 10 of f_5x11). f_wide's raggedness is
    # in the frame, not in the grid -- i / 4 never passes g_lr - 1 there, the two maps are the same map -- and f_8x12 is exact
    ragged = l.grid[0] % 4 != 0 or l.grid[1] % 4 != 0
    assert ragged == (l.name in ("f_11x5", "f_5x11"))
    assert (differs["modulo"] > 0) == ragged
    # per pair: the pair offset matters in every pair after the first
    for k in (1, 2):
        assert (_mutant(l, s.coarse64, "pair0")[k] != right[k]).any(), k


def test_a_uniform_scene_would_hide_every_wrong_map():
    """the counter-proof: the same check on a field whose cells all move alike sees nothing -- what every coarse-to-fine test stood on"""
    l = FC.BY_NAME["f_8x12"]
    coarse = np.broadcast_to(np.array([6.03, -4.8]), (FC.N_PAIRS, 6, 2)).copy()
    right = _mutant(l, coarse, "right")
    assert right.any()
    for which in ("transposed", "swapped", "divisor", "pair0", "modulo"):
        assert np.array_equal(_mutant(l, coarse, which), right), which


@pytest.mark.parametrize("l", FC.FIELDS, ids=lambda l: l.name)
def test_inside_patches_are_many_clear_and_on_the_fast_path(l):
    """B.5 - B.7"""
    s = FC.scene(l.name)
    assert np.array_equal(s.pred, PC.c2f_pred_np(l, s.coarse64)) and np.array_equal(s.applied, PC.applied_np(l, s.pred))
    counts = []
    for k in range(FC.N_PAIRS):
        cn = FC.counted(s, k)
        ins = int((s.inside[k] & cn).sum())
        counts.append(f"{ins}/{int(cn.sum())}")
        assert 2 * ins >= int(cn.sum()), (k, ins, int(cn.sum()))
    assert s.clear[s.inside].all(), np.argwhere(s.inside & ~s.clear).tolist()
    dd = np.abs(s.w64 - s.w32).max(axis=-1)
    assert np.isfinite(dd[s.inside]).all() and np.isnan(dd[~s.inside]).all()
    print(f"{l.name}: inside patches per pair {' '.join(counts)} (+ {int((s.inside[1] & ~FC.counted(s, 1)).sum())} of the identical cell); "
          f"oracle distance on them, worst {dd[s.inside].max():.2e} px; residuals up to {np.abs(s.w64[s.inside]).max():.2f} px")
    assert dd[s.inside].max() <= tolerances.F32_LIMITED_FROM
    # an inside patch sees one texture under one shift: the residual is what the prediction left of the planted shift, under a pixel off
    # the integer (the 5 x 5 centroid of a non-periodic shift is biased towards 0: test_fft_pred_host.py) -- a statement about the
    # integer peak, which the GPU test never uses
    for k, p in np.argwhere(s.inside):
        kind, dx, dy = s.kinds[k][FC.cell_of(l, p)]
        assert np.abs(s.w64[k, p] - ((dx, dy) - s.applied[k, p])).max() < 1.0, (k, p)


@pytest.mark.parametrize("l", FC.FIELDS, ids=lambda l: l.name)
def test_gate_pair_has_a_gap_of_a_factor_two(l):
    """C.6's input: the cell with unrelated previous content answers with less than half the response of any other cell, the threshold
    lies between, and the other cells predict off every tie"""
    g = FC.gate_case(l.name)
    others = np.delete(g.responses, FC.GATE_CELL)
    print(f"{l.name}: long-range responses {np.round(g.responses, 3).tolist()}, threshold {g.threshold:.3f}")
    assert others.min() > 0 and others.min() >= 2.0 * g.responses[FC.GATE_CELL]
    assert g.responses[FC.GATE_CELL] < g.threshold < others.min()
    assert g.threshold - g.responses[FC.GATE_CELL] > 0.05 and others.min() - g.threshold > 0.05  # (far from a kernel's 1e-6 of the oracle)
    keep = np.delete(g.coarse64[0], FC.GATE_CELL, axis=0)
    assert not np.isnan(keep).any() and _tie(keep) <= TIE
    preds = [PC.round4_np(*v) for v in keep]
    assert len(set(preds)) == len(preds) and all(p[0] != 0 and p[1] != 0 for p in preds)


# ---- coarse to fine on every pair route ----
@pytest.mark.parametrize("n", FC.ROUTE_SIZES)
def test_route_case_conditions(n):
    """the recorded table names the kernel and whether a fused form exists; the oracles predict alike and off every tie; the clamp holds
    back column 0 and row 3 and nothing else; every patch whose clamp is inactive has a clear peak, and every patch with a clear peak lies
    on the fast path of tests/tolerances.py"""
    r = FC.route_case(n)
    l = r.layout
    row = FC.route_row(n)
    want = {64: ("stockham", True), 120: ("planned-half", True), 128: ("stockham", True), 96: ("planned-half", True), 160: ("planned-half", True),
            62: ("planned", False), 200: ("planned-large", False), 57: ("planned-half", True), 24: ("planned", False)}[n]
    assert (l.variant, FC.route_fused(n)) == want, (row, l.variant, FC.route_fused(n))
    assert l.grid == (4, 4) and l.w == l.h == 4 * n and r.cur.shape == (FC.ROUTE_PAIRS, 4 * n, 4 * n) and not np.array_equal(r.cur[0], r.cur[1])
    assert r.coarse64.shape == (FC.ROUTE_PAIRS, 1, 2)
    assert np.array_equal(PC.c2f_pred_np(l, r.coarse64), PC.c2f_pred_np(l, r.coarse32)) and _tie(r.coarse64) <= TIE and _tie(r.coarse32) <= TIE
    assert np.abs(r.coarse64 - r.coarse32).max() <= tolerances.F32_LIMITED_FROM
    assert FC.route_clamped(n) == 7 and ((~r.free).sum(axis=1) == 7).all()
    assert r.clear[r.free].all()
    dd = np.abs(r.w64 - r.w32).max(axis=-1)
    assert dd[r.clear].max() <= tolerances.F32_LIMITED_FROM
    print(f"n={n} {l.variant}: predictions {r.pred[:, 0].tolist()}, tie margin {_tie(r.coarse64):.3f}, {int((~r.clear).sum())} of the 14 clamped patches "
          f"without a clear peak, oracle distance {dd[r.clear].max():.2e} px")


def test_route_sizes_cover_every_pair_route():
    """one size per kernel variant a pair launch can take, the reference geometry 480 / 120 among them"""
    assert FC.ROUTE_SIZES == [64, 120, 128, 96, 160, 62, 200, 57, 24]
    assert {FC.route_layout(n).variant for n in FC.ROUTE_SIZES} == {"stockham", "planned", "planned-half", "planned-large"}
    assert {R.route_class(FC.route_row(n))[0] for n in FC.ROUTE_SIZES} == {"TUNED", "PLANNED", "LARGE"}
    # half-tile forms: equal to the transform size (96, 120, 160) and padded (57 -> 60)
    assert FC.route_row(57)[2] == 60 and [FC.route_row(n)[2] for n in (96, 120, 160)] == [96, 120, 160]
