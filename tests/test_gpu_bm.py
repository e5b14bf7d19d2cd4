"""GPU parity tests of K2/K3 (SAD block scan + histogram mode) through the C ABI. Integer work:
every comparison with the CPU oracle is bit-exact."""
import os

import numpy as np
import pytest
import torch

import oracle_lib as O
from mrs_optic_flow_amd import BlockMethod, FastSpacedBMMethod, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["bm_fast_spaced_c3.npz", "bm_block_method_c1.npz"])
def test_golden_vectors(gpu, name):
    g = np.load(os.path.join(GOLDEN, name))
    block, step, radius, fast = (int(v) for v in g["params"])
    h, w = g["cur"].shape[1:]
    eng = FastSpacedBMMethod(block, radius, step, (h, w)) if fast else BlockMethod(h, block, radius)
    dx, dy, mode = eng.process_batch_host(g["cur"], g["prev"])
    assert (dx == g["dx"]).all() and (dy == g["dy"]).all()
    assert (mode[:, :2] == g["mode"]).all()
    assert (mode[:, 0:6:2] == g["top"][:, 0]).all() and (mode[:, 1:6:2] == g["top"][:, 1]).all()


@pytest.mark.parametrize("fast,shape,block,step,radius", [
    (True, (480, 752), 16, 8, 16),    # BASELINE c3
    (False, (272, 272), 32, 0, 8),    # BASELINE c1 (crop 272^2, 8x8 blocks of 32, +-8)
    (True, (100, 140), 8, 4, 5),
    (False, (120, 120), 16, 0, 21),   # default.yaml scan_radius 21
    (True, (150, 150), 64, 0, 3),     # >256 px per block: u16 partial sums are flushed
    # the reference's OWN default geometry (config/default.yaml:29-32: scan_radius 21, step_size 24, sample_point_size
    # 120) on the 752x480 camera frame and on the 480^2 crop the node hands its processors
    (True, (480, 752), 120, 24, 21),
    (True, (480, 480), 120, 24, 21),
    (False, (480, 480), 120, 0, 21),  # BlockMethod(frame_size 480, sample_point_size 120, scan_radius 21): 3 x 3 blocks
    (True, (400, 300), 128, 0, 24),   # the largest block size, at the reference's radius limit (2r + 1 <= 50, .cl:1)
    (True, (230, 420), 100, 4, 48),   # > 64 KB of LDS per workgroup: opt-in dynamic LDS
    (True, (60, 200), 8, 0, 2),       # tiny scans: eight blocks share a workgroup
    # row lengths that no chunk length of the generic scan divides (ragged row tails of 1, 3, 5 and 1 dwords) and odd radii
    (True, (200, 330), 36, 4, 7),
    (True, (180, 300), 44, 0, 9),
    (False, (250, 250), 52, 0, 11),
    (True, (330, 420), 100, 8, 13),
    (True, (300, 300), 124, 0, 5),
    (True, (90, 200), 12, 4, 3),
    (True, (90, 230), 20, 0, 6),
])
def test_seeded_batches_bit_exact(gpu, fast, shape, block, step, radius):
    h, w = shape
    B = 5
    cur, prev, shifts, kinds = synth.batch_np(B, h, w, min(radius - 2, 12), k0=0)
    if fast:
        eng, cfg = FastSpacedBMMethod(block, radius, step, shape), O.bm_config_fast_spaced(w, h, block, step, radius)
    else:
        eng, cfg = BlockMethod(h, block, radius), O.bm_config_block_method(h, block, radius)
    assert (eng.cfg.grid_x, eng.cfg.grid_y) == (cfg.grid_x, cfg.grid_y)
    dx, dy, mode = eng.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu))
    dx, dy, mode = dx.cpu().numpy(), dy.cpu().numpy(), mode.cpu().numpy()
    for k in range(B):
        wdx, wdy, wmode = O.bm_process(cur[k], prev[k], cfg)
        assert (dx[k] == wdx).all() and (dy[k] == wdy).all(), (k, kinds[k])
        assert tuple(mode[k, :2]) == wmode
        assert list(mode[k, 0:6:2]) == list(O.bm_histogram_top(wdx, radius, 3))
        assert list(mode[k, 1:6:2]) == list(O.bm_histogram_top(wdy, radius, 3))
        if kinds[k] == "shift":
            assert wmode == (-shifts[k][0], -shifts[k][1])  # block matching reports the opposite sign


def test_ties_and_low_contrast_rule(gpu):
    f = np.full((112, 112), 90, np.uint8)
    dx, dy, mode = BlockMethod(112, 32, 8).process_batch_host(f[None], f[None])
    assert (dx == -8).all() and (dy == -8).all() and tuple(mode[0, :2]) == (-8, -8)  # BlockMethod.cpp:63 first min
    dx, dy, mode = FastSpacedBMMethod(16, 8, 8, (112, 112)).process_batch_host(f[None], f[None])
    assert (dx == 0).all() and (dy == 0).all()                                      # FastSpacedBMMethod.cl:77-82
    rng = np.random.default_rng(7)
    for _ in range(8):  # tiny alphabet -> many exact ties; the first minimum in row-major order must win
        prev = rng.integers(0, 3, (40, 40), dtype=np.uint8)
        cur = rng.integers(0, 3, (40, 40), dtype=np.uint8)
        cfg = O.bm_config_block_method(40, 8, 4)
        dx, dy, _ = BlockMethod(40, 8, 4).process_batch_host(cur[None], prev[None])
        wdx, wdy, _ = O.bm_process(cur, prev, cfg)
        assert (dx[0] == wdx).all() and (dy[0] == wdy).all()
    r, b = 5, 8  # threshold 5.0 exactly: gap 5 zeroed, gap 6 kept (double compare, .cl:2)
    size = b + 2 * r
    for gap in (5, 6):
        prev = np.full((size, size), 100, np.uint8)
        prev[r, r] = 100 + gap
        cur = np.full((size, size), 100, np.uint8)
        dx, dy, _ = FastSpacedBMMethod(b, r, 0, (size, size)).process_batch_host(cur[None], prev[None])
        wdx, wdy, _ = O.bm_process(cur, prev, O.bm_config_fast_spaced(size, size, b, 0, r))
        assert (dx[0] == wdx).all() and (dy[0] == wdy).all()


def test_stateful_processimage(gpu):
    """prev starts as zeros (BlockMethod.cpp:17-18), then prev <- cur after every call (:89)."""
    fs = 144
    seq = [synth.pair_np(5, fs, fs, 2 * t, -t, blur=False)[0] for t in range(3)]
    eng = BlockMethod(fs, 32, 8)
    cfg = O.bm_config_block_method(fs, 32, 8)
    prev = np.zeros((fs, fs), np.uint8)
    for f in seq:
        dx, dy, mode = eng.processBlocks(f)
        wdx, wdy, wmode = O.bm_process(f, prev, cfg)
        assert (dx == wdx).all() and (dy == wdy).all() and mode == wmode
        prev = f
    assert eng.processImage(seq[0]).shape == (1, 2)


def test_full_size_c3_batch_properties(gpu):
    """BASELINE c3 at full size (752x480, sps 16, step 8, r 16, batch 1024)."""
    B, h, w = 1024, 480, 752
    cur, prev, shifts, kinds = synth.batch_torch(B, h, w, 12, gpu)
    eng = FastSpacedBMMethod(16, 16, 8, (h, w))
    dx, dy, mode = eng.process_batch_device(cur, prev)
    torch.cuda.synchronize()
    dx, dy, mode, sh = dx.cpu().numpy(), dy.cpu().numpy(), mode.cpu().numpy(), shifts.numpy()
    for k in range(B):
        if kinds[k] == "shift":
            assert (dx[k] == -sh[k, 0]).all() and (dy[k] == -sh[k, 1]).all()  # SAD 0 at the planted offset
            assert tuple(mode[k, :2]) == (-sh[k, 0], -sh[k, 1])
        elif kinds[k] in ("identical", "constant"):
            assert (dx[k] == 0).all() and (dy[k] == 0).all()
    cfg = O.bm_config_fast_spaced(w, h, 16, 8, 16)
    for k in (11, 531):  # noisy pairs against the oracle
        wdx, wdy, wmode = O.bm_process(cur[k].cpu().numpy(), prev[k].cpu().numpy(), cfg)
        assert (dx[k] == wdx).all() and (dy[k] == wdy).all() and tuple(mode[k, :2]) == wmode


def test_random_geometries_bit_exact(gpu):
    """Seeded sweep over block sizes / steps / radii / frame sizes (fast 16x16 path and the generic kernel)."""
    rng = np.random.default_rng(20261003)
    for trial in range(24):
        block = int(rng.choice([4, 8, 12, 16, 16, 16, 20, 32, 72, 120]))
        radius = int(rng.choice([2, 5, 8, 8, 16, 16, 21])) if block != 16 else int(rng.choice([8, 16, 16, 5]))
        step = int(rng.choice([0, 4, 8, 3])) if block != 16 else int(rng.choice([0, 4, 8, 12]))
        gx, gy = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        S = block + step
        w = gx * S + 2 * radius + int(rng.integers(0, S))  # reference grid maths: (w - 2r) / S = gx
        h = gy * S + 2 * radius + int(rng.integers(0, S))
        cur = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        prev = np.roll(cur, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(1, 2))
        prev = np.clip(prev.astype(np.int32) + rng.integers(-6, 7, prev.shape), 0, 255).astype(np.uint8)
        eng = FastSpacedBMMethod(block, radius, step, (h, w))
        cfg = O.bm_config_fast_spaced(w, h, block, step, radius)
        assert (eng.cfg.grid_x, eng.cfg.grid_y) == (cfg.grid_x, cfg.grid_y)
        dx, dy, mode = eng.process_batch_host(cur, prev)
        for k in range(2):
            wdx, wdy, wmode = O.bm_process(cur[k], prev[k], cfg)
            assert (dx[k] == wdx).all() and (dy[k] == wdy).all(), (trial, block, step, radius, w, h)
            assert tuple(mode[k, :2]) == wmode


@pytest.mark.parametrize("block,step,radius", [(16, 8, 16), (16, 4, 8), (24, 4, 5), (120, 24, 21), (32, 0, 8), (12, 4, 3)])
def test_bgr_front_end_fused_into_the_block_scans(gpu, block, step, radius):
    """SURVEY N2 for K2: interleaved BGR8 camera frames (a crop of a larger frame, odd byte offsets), CV_RGB2GRAY as the node
    applies it (optic_flow.cpp:1622) inside the staging loads of both scan kernels: the same bits as the gray entry on the
    converted crop, and the oracle's shifts."""
    B, h, w, xi, yi = 3, 150 + 2 * radius, 260 + 2 * radius, 7, 5
    if block == 120:
        h, w = 330, 480
    H, W = h + 11, w + 19
    rng = np.random.default_rng(block * 100 + radius)
    base = [synth.pair_np(30 + k, H, W, 2 + k, -k) for k in range(B)]

    def colour(g):
        g = g.astype(np.int32)
        ch = np.stack([g, 255 - g // 2, (g * 3 // 4 + 20)], axis=-1) + rng.integers(-2, 3, g.shape + (3,))
        return np.clip(ch, 0, 255).astype(np.uint8)
    cur = np.stack([colour(c) for c, _ in base])
    prev = np.stack([colour(p) for _, p in base])
    eng = FastSpacedBMMethod(block, radius, step, (h, w))
    cfg = O.bm_config_fast_spaced(w, h, block, step, radius)
    tc, tp = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    dx, dy, mode = eng.process_batch_device_bgr(tc[:, yi:yi + h, xi:xi + w], tp[:, yi:yi + h, xi:xi + w])
    dx, dy, mode = dx.cpu().numpy(), dy.cpu().numpy(), mode.cpu().numpy()
    for k in range(B):
        gc, gp = O.rgb2gray(cur[k, yi:yi + h, xi:xi + w]), O.rgb2gray(prev[k, yi:yi + h, xi:xi + w])
        wdx, wdy, wmode = O.bm_process(gc, gp, cfg)
        assert (dx[k] == wdx).all() and (dy[k] == wdy).all() and tuple(mode[k, :2]) == wmode, k
        gx, gy, gm = eng.process_batch_device(torch.from_numpy(gc[None]).to(gpu), torch.from_numpy(gp[None]).to(gpu))
        assert torch.equal(gx[0].cpu(), torch.from_numpy(dx[k])) and torch.equal(gy[0].cpu(), torch.from_numpy(dy[k]))
        assert np.array_equal(gm[0].cpu().numpy(), mode[k])


def test_refine_matches_oracle(gpu):
    """mof_bm_refine (BlockMethod::Refine, faithful and repaired) on the frames of the last processImage call."""
    fs = 144
    seq = [synth.pair_np(81, fs, fs, -3 * t, 2 * t)[0] for t in range(3)]
    eng = BlockMethod(fs, 32, 8)
    eng.processBlocks(seq[0])
    for t in (1, 2):
        dx, dy, mode = eng.processBlocks(seq[t])
        for faithful in (True, False):
            for fp in (mode, (0, 0), (-2, -1), (3, -4)):
                want = O.bm_refine(seq[t], seq[t - 1], fp, 2, faithful)
                assert eng.refine(fp, 2, faithful) == want, (t, faithful, fp)
    from mrs_optic_flow_amd import MofError
    with pytest.raises(MofError):
        eng.refine((400, 0))


@pytest.mark.parametrize("radius", [2, 4, 6, 8, 10, 12, 14, 16])
def test_fast_16x16_scan_at_every_even_radius(gpu, radius):
    """r06: bm_scan16_kernel<R> (blocks of 16 x 16, v_qsad_pk_u16_u8 on register-resident blocks) serves every even scan radius up to 16,
    not only c3's 8 and 16. Bit-exact against the oracle on random frames with ties (small alphabet), the low-contrast rule on, steps 0 / 4 / 8,
    block rows that fill a wave exactly, spill into a second one, or hold a single block; gray and BGR8."""
    rng = np.random.default_rng(100 + radius)
    for step, gx, gy, extra in ((0, 1, 1, 0), (4, 5, 2, 3), (8, 64 // max(1, radius // 2) + 1, 1, 7), (8, 3, 3, 0), (0, 9, 2, 11)):
        S = 16 + step
        w, h = gx * S + 2 * radius + extra % S, gy * S + 2 * radius + (extra % 5)  # (FastSpacedBMMethod_OCL.cpp:82-90: (size - 2 r) / S blocks per axis)
        levels = 256 if step else 4  # (a four-level alphabet: many exact ties, the first minimum in row-major order must win)
        cur = rng.integers(0, levels, (3, h, w), dtype=np.uint8)
        prev = np.roll(cur, (int(rng.integers(-2, 3)), int(rng.integers(-2, 3))), axis=(1, 2))
        prev = np.clip(prev.astype(np.int32) + rng.integers(-1, 2, prev.shape), 0, 255).astype(np.uint8)
        eng = FastSpacedBMMethod(16, radius, step, (h, w))
        assert (eng.cfg.grid_x, eng.cfg.grid_y) == (gx, gy), (eng.cfg.grid_x, eng.cfg.grid_y, gx, gy)
        cfg = O.bm_config_fast_spaced(w, h, 16, step, radius)
        dx, dy, mode = (v.cpu().numpy() for v in eng.process_batch_device(torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)))
        for k in range(3):
            wdx, wdy, wmode = O.bm_process(cur[k], prev[k], cfg)
            assert (dx[k] == wdx).all() and (dy[k] == wdy).all() and tuple(mode[k, :2]) == wmode, (radius, step, gx, gy, k)


# ---- saturated content: every 16-bit field of a packed SAD above 2^15 (tests/hard_content.py) --------------------------------------------
# v_qsad_pk_u16_u8 accumulates into four 16-bit fields; "255 * 256 < 65536" is why that is exact. Noise against noise stays near 85 per pixel
# (about 21,850 per 256 pixels, sigma about 960: bit 15 is never set), so the flush interval of the generic scan, the packed (sad << 16 | index)
# key of the 16 x 16 scan and the centre - best difference of the low-contrast rule only ever saw the lower half of their range.
SATURATED_GEOMETRIES = [
    (16, 0, 2), (16, 8, 2), (16, 0, 8), (16, 8, 8), (16, 0, 16), (16, 8, 16),  # the 16 x 16 form
    (8, 0, 2), (8, 4, 5),      # generic form, eight blocks per workgroup (64-pixel blocks: their sums cannot reach 2^15)
    (32, 0, 8),
    (36, 4, 7), (44, 0, 9),    # ragged row tails
    (64, 0, 3), (100, 4, 13),  # packed sums flushed every 4 and 2 rows
    (120, 24, 21), (128, 0, 24),
]


def _low_contrast_gap(radius):
    return int(np.floor(0.2 * radius * radius))  # the largest centre - best that FastSpacedBMMethod.cl:77-82 still zeroes


def _saturated_frames(block, step, radius):
    """(names, cur[n, h, w], prev[n, h, w], planted shift) for a 3 x 2 grid of blocks (and some slack, so the frame is wider than high)."""
    import hard_content as H

    S, r = block + step, radius
    h, w = 2 * S + 2 * r + 1, 3 * S + 2 * r + 5 + (6 * S if block == 8 else 0)  # (block 8: nine blocks a row, more than one workgroup takes)
    seed = 1000 * block + 10 * radius + step
    names, cur, prev = [], [], []
    c, p = H.band_pair(seed, (h, w), 40)
    names += ["band_pair(40)", "band_pair(40) swapped"]
    cur += [c, p]
    prev += [p, c]
    black, white = np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)
    names += ["0 against 255", "255 against 0"]
    cur += [black, white]
    prev += [white, black]
    # binary noise with a planted shift: cur[y, x] = prev[y - sy, x - sx] -> SAD 0 at candidate (-sx, -sy), multiples of 255 elsewhere
    sx, sy = min(r, 3) - (r > 1), -(min(r, 5) // 2)
    pn = H.binary_noise(seed, (h, w))
    names.append("binary noise, planted shift")
    cur.append(np.roll(pn, (sy, sx), axis=(0, 1)))
    prev.append(pn)
    # 0 / 255 noise of density q against black, q chosen so that the sums over TWICE the pixels of one 16-bit field (two flush intervals of
    # the generic scan; 512 pixels where a block is one field) lie around 2^16: mean 65536, sigma about 2800. The fields themselves then
    # lie around 2^15 and are exact; summed over any longer interval about half the candidates would wrap and half would not. (On the other
    # frames of this list every candidate's sum over two intervals lies in [2^16, 2^17): a 16-bit wrap takes the same 65536 off all of
    # them and leaves every answer as it was -- these frames are what a flush interval that is too long cannot survive.)
    field_px = block * (block if block <= 16 else max(256 // block, 1))
    names.append("noise around 2^16 per two fields")
    cur.append(black)
    prev.append(H.bernoulli_noise(seed, (h, w), 65536.0 / (255.0 * 2 * field_px) if field_px >= 188 else 0.5))
    # the low-contrast threshold straddled at saturated magnitude: from 0 against 255, ONE pixel per block -- a corner of its window, which
    # only the corner candidate of that block covers -- is lowered, so that candidate beats the centre by exactly that much: by `gap` in
    # the first block row (top-left corners: no window of the second row reaches them) and by gap + 1 in the second (bottom-right corners,
    # below every window of the first row). The planted pixels of a row are a whole block pitch apart: no candidate covers two.
    gap = _low_contrast_gap(r)
    assert gap + 1 <= 255
    pl = white.copy()
    gx, gy = (w - 2 * r) // S, (h - 2 * r) // S
    W = block + 2 * r
    assert gy == 2
    for bx in range(gx):
        pl[0, bx * S] = 255 - gap
        pl[S + W - 1, bx * S + W - 1] = 255 - (gap + 1)
    names.append("threshold straddled")
    cur.append(black)
    prev.append(pl)
    return names, np.stack(cur), np.stack(prev), (sx, sy)


def _check_saturated(gpu, block, step, radius, bgr=True):
    """The body of test_saturated_sads_bit_exact (a child process runs it too, under MOF_BM_GENERIC=1)."""
    names, cur, prev, (sx, sy) = _saturated_frames(block, step, radius)
    n, h, w = cur.shape
    S, r, D = block + step, radius, 2 * radius + 1
    # the derivation, on one block with numpy: every candidate's SAD over the pixels the kernels keep in one 16-bit field (the whole 16 x 16
    # block; 256 // block rows of a larger one) lies in [175 n, 255 n] -- [44800, 65280] for 256 pixels: bit 15 set, 16 bits kept
    rows = block if block <= 16 else max(256 // block, 1)
    c0 = cur[0, r:r + block, r:r + block].astype(np.int64)
    full = np.zeros((D, D), np.int64)
    for ys in range(D):
        for xs in range(D):
            d = np.abs(c0 - prev[0, ys:ys + block, xs:xs + block].astype(np.int64))
            full[ys, xs] = d.sum()
            for j0 in range(0, block - rows + 1, rows):
                f, npx = int(d[j0:j0 + rows].sum()), rows * block
                assert 175 * npx <= f <= 255 * npx and f < 1 << 16, (block, ys, xs, j0, f)
                assert npx < 188 or f & 0x8000, (block, ys, xs, j0, f)
    assert block == 8 or rows * block >= 188  # (only the 64-pixel blocks stay below 2^15)
    srt = np.sort(full.ravel())
    assert srt[0] < srt[1], "the minimum of a band_pair block is not unique"

    tc, tp = torch.from_numpy(cur).to(gpu), torch.from_numpy(prev).to(gpu)
    engines = [("fast", FastSpacedBMMethod(block, radius, step, (h, w)), O.bm_config_fast_spaced(w, h, block, step, radius), slice(0, w))]
    if step == 0:  # BlockMethod: square frames, no low-contrast rule
        engines.append(("block", BlockMethod(h, block, radius), O.bm_config_block_method(h, block, radius), slice(0, h)))
    checked = 0
    for kind, eng, cfg, cols in engines:
        assert (eng.cfg.grid_x, eng.cfg.grid_y) == (cfg.grid_x, cfg.grid_y)
        dx, dy, mode = (v.cpu().numpy() for v in eng.process_batch_device(tc[:, :, cols], tp[:, :, cols]))
        zeroed = kept = 0
        for k in range(n):
            ck, pk = np.ascontiguousarray(cur[k][:, cols]), np.ascontiguousarray(prev[k][:, cols])
            wdx, wdy, wmode = O.bm_process(ck, pk, cfg)
            wdx, wdy = wdx.reshape(dx[k].shape), wdy.reshape(dy[k].shape)
            bad = np.argwhere((dx[k] != wdx) | (dy[k] != wdy))
            if bad.size:
                b0 = tuple(int(v) for v in bad[0])
                raise AssertionError((kind, names[k], (block, step, radius), f"{len(bad)} blocks differ; first (by, bx) {b0}: got "
                                      f"{(int(dx[k][b0]), int(dy[k][b0]))}, want {(int(wdx[b0]), int(wdy[b0]))}"))
            assert tuple(mode[k, :2]) == wmode, (kind, names[k])
            assert list(mode[k, 0:6:2]) == list(O.bm_histogram_top(wdx, radius, 3)), (kind, names[k])
            assert list(mode[k, 1:6:2]) == list(O.bm_histogram_top(wdy, radius, 3)), (kind, names[k])
            checked += 1
            # what the answers must be, oracle or not
            if names[k] in ("0 against 255", "255 against 0"):  # every SAD = 255 block^2: all ties
                want = 0 if kind == "fast" else -r              # the low-contrast rule / the first minimum (BlockMethod.cpp:63)
                assert (dx[k] == want).all() and (dy[k] == want).all(), (kind, names[k])
            elif names[k].startswith("binary noise"):
                assert (dx[k] == -sx).all() and (dy[k] == -sy).all(), (kind, names[k], sx, sy)
            elif names[k] == "threshold straddled" and kind == "fast":
                zeroed, kept = int(((dx[k] == 0) & (dy[k] == 0)).sum()), int(((dx[k] != 0) | (dy[k] != 0)).sum())
        if kind == "fast":
            assert zeroed == kept == cfg.grid_x, (zeroed, kept)  # first block row zeroed, second kept: both sides of the threshold
    # the threshold on ONE block, each corner of its window in turn (first and last x-shift, first and last y-shift): lowered by gap ->
    # zeroed; by gap + 1 -> the corner candidate is kept
    size, gap = block + 2 * r, _low_contrast_gap(r)
    one = FastSpacedBMMethod(block, radius, 0, (size, size))
    cz = np.zeros((size, size), np.uint8)
    for oy, ox in ((0, 0), (0, size - 1), (size - 1, 0), (size - 1, size - 1)):
        for g in (gap, gap + 1):
            pv = np.full((size, size), 255, np.uint8)
            pv[oy, ox] = 255 - g
            assert block == 8 or 255 * block * block - g > 1 << 15
            want = (0, 0) if g == gap else (r if ox else -r, r if oy else -r)
            dx, dy, _ = (v.cpu().numpy() for v in one.process_batch_device(torch.from_numpy(cz[None]).to(gpu), torch.from_numpy(pv[None]).to(gpu)))
            wdx, wdy, _ = O.bm_process(cz, pv, O.bm_config_fast_spaced(size, size, block, 0, r))
            assert (int(dx.ravel()[0]), int(dy.ravel()[0])) == want == (int(wdx.ravel()[0]), int(wdy.ravel()[0])), (g, oy, ox, dx, dy, wdx, wdy)
    # the BGR8 entry: white BGR must give gray 255 (and black 0), then the same bits as the gray entry
    if bgr:
        assert (O.rgb2gray(np.full((4, 8, 3), 255, np.uint8)) == 255).all() and (O.rgb2gray(np.zeros((4, 8, 3), np.uint8)) == 0).all()
        kind, eng, cfg, cols = engines[0]
        bc, bp = (np.ascontiguousarray(np.repeat(a[..., None], 3, axis=-1)) for a in (cur, prev))
        gdx, gdy, gmode = (v.cpu().numpy() for v in eng.process_batch_device(tc, tp))
        dx, dy, mode = (v.cpu().numpy() for v in eng.process_batch_device_bgr(torch.from_numpy(bc).to(gpu), torch.from_numpy(bp).to(gpu)))
        for k in range(n):
            assert np.array_equal(O.rgb2gray(bc[k]), cur[k]) and np.array_equal(O.rgb2gray(bp[k]), prev[k]), names[k]
            assert np.array_equal(dx[k], gdx[k]) and np.array_equal(dy[k], gdy[k]) and np.array_equal(mode[k], gmode[k]), ("bgr", names[k])
    return checked


@pytest.mark.parametrize("block,step,radius", SATURATED_GEOMETRIES)
def test_saturated_sads_bit_exact(gpu, block, step, radius):
    """Both scans on frames whose partial sums fill their 16-bit fields (band_pair(40): every 256-pixel SAD in [44800, 65280], asserted with
    numpy on one block), on the extremes (0 against 255 and back: every SAD = 255 block^2, all ties -> BlockMethod's first minimum (-r, -r),
    FastSpacedBMMethod's (0, 0) by the low-contrast rule), on binary noise with a planted shift (SAD 0 there, multiples of 255 elsewhere), on 0 / 255
    noise whose sums over two flush intervals lie around 2^16 (a longer interval would wrap half the candidates) and on the low-contrast threshold straddled at that magnitude (centre - best = floor(0.2 r^2) and one more, both sums above 2^15): bit-exact
    against the oracle, gray and BGR8."""
    assert _check_saturated(gpu, block, step, radius) >= 7


_GENERIC16_SCRIPT = r"""
import sys
sys.path[:0] = [{root!r}, {tests!r}]
import torch
import test_gpu_bm as T
dev = torch.device("cuda", 0)
checked = 0
for block, step, radius in T.SATURATED_GEOMETRIES:
    if block == 16:
        checked += T._check_saturated(dev, block, step, radius)
print("generic16 ok", checked)
"""


def test_block_16_on_the_generic_scan_with_saturated_sads(gpu):
    """MOF_BM_GENERIC=1 sends 16 x 16 blocks through the generic scan (the knob is read once per process): the saturated cases of the
    16 x 16 geometries once more in a child process with the knob set; MOF_BM_VERBOSE shows that the generic form really ran."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = _GENERIC16_SCRIPT.format(root=root, tests=os.path.join(root, "tests"))
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MOF_BM_GENERIC="1", MOF_BM_VERBOSE="1"))
    n16 = sum(1 for g in SATURATED_GEOMETRIES if g[0] == 16)
    assert r.returncode == 0 and f"generic16 ok {n16 * 7 + 3 * 7}" in r.stdout, (r.stdout[-1500:], r.stderr[-1500:])
    assert "block scan plan" in r.stderr, r.stderr[-500:]
