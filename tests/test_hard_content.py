"""CPU tests of tests/hard_content.py (numpy only): the generators are seeded and have the properties the GPU tests lean on."""
import numpy as np
import pytest

import hard_content as H


def test_generators_are_seeded_and_full_range():
    for make in (H.binary_noise, H.uniform_noise, H.impulses, H.holes):
        a, b, c = make(5, (96, 120)), make(5, (96, 120)), make(6, (96, 120))
        assert a.dtype == np.uint8 and a.shape == (96, 120)
        assert np.array_equal(a, b) and not np.array_equal(a, c), make.__name__
    for lo in (0, 40):
        (c1, p1), (c2, p2), (c3, p3) = H.band_pair(9, 64, lo), H.band_pair(9, 64, lo), H.band_pair(10, 64, lo)
        assert np.array_equal(c1, c2) and np.array_equal(p1, p2) and c1.dtype == p1.dtype == np.uint8
        assert lo == 0 or not (np.array_equal(c1, c3) or np.array_equal(p1, p3))
    assert set(np.unique(H.binary_noise(1, 240))) == {0, 255}
    assert 0.49 < (H.binary_noise(1, 240) == 255).mean() < 0.51
    u = H.uniform_noise(1, 240)
    assert u.min() == 0 and u.max() == 255 and len(np.unique(u)) == 256
    assert np.array_equal(H.binary_noise(3, 64), H.binary_noise(3, (64, 64)))  # an int is a square


@pytest.mark.parametrize("shape", [96, 120, 200, 240, 256, 480, (100, 141)])
@pytest.mark.parametrize("pitch", [12, 9])
def test_impulses_are_isolated_and_reach_the_border(shape, pitch):
    for seed in range(4):
        img = H.impulses(seed, shape, pitch)
        h, w = img.shape
        assert set(np.unique(img)) == {0, 255}
        ys, xs = np.nonzero(img)
        pos = H.impulse_positions(seed, shape, pitch)
        assert len(pos) == len(ys) == len({tuple(p) for p in pos})
        # no two impulses inside one FOOTPRINT x FOOTPRINT window: for every pair, |dy| or |dx| is at least the pitch (> the footprint)
        dy, dx = np.abs(ys[:, None] - ys[None, :]), np.abs(xs[:, None] - xs[None, :])
        far = np.maximum(dy, dx) + np.eye(len(ys), dtype=np.int64) * 10 ** 6
        assert far.min() >= pitch > H.FOOTPRINT, (seed, far.min())
        # the rows and columns that reflect-101 taps land on are populated, and so is the interior
        for line in (0, 1, h - 2, h - 1):
            assert img[line].any(), (seed, "row", line)
        for line in (0, 1, w - 2, w - 1):
            assert img[:, line].any(), (seed, "column", line)
        assert int((img[2:-2, 2:-2] == 255).sum()) >= ((h - 4 * pitch) // pitch) * ((w - 4 * pitch) // pitch) >= 1
        assert np.array_equal(H.holes(seed, shape, pitch), 255 - img)
    with pytest.raises(ValueError):
        H.impulses(0, 240, H.FOOTPRINT)


def test_periodic_and_split_images():
    c1, c2 = H.checker(16, 1), H.checker(16, 2)
    assert set(np.unique(c1)) == {0, 255} and c1[0, 0] == 0 and c1[0, 1] == 255 and c1[1, 0] == 255
    assert np.array_equal(c1[:-1, :-1], 255 - c1[1:, :-1]) and np.array_equal(c1[:, :-1], 255 - c1[:, 1:])
    assert np.array_equal(c2[::2, ::2], c1[:8, :8]) and np.array_equal(c2[1::2, 1::2], c1[:8, :8])
    assert np.array_equal(H.checker(16, 1, 1), 255 - c1)
    sc, sr = H.stripes((8, 12), 1), H.stripes((8, 12), 0)
    assert (sc == sc[0]).all() and list(sc[0, :4]) == [0, 255, 0, 255]
    assert (sr == sr[:, :1]).all() and list(sr[:4, 0]) == [0, 255, 0, 255]
    for res in (96, 200, 240):
        v, hz = H.halves(res, 1), H.halves(res, 0)
        c = res // 2  # the log-polar centre: the first white column / row
        assert (v[:, :c] == 0).all() and (v[:, c:] == 255).all() and (hz[:c] == 0).all() and (hz[c:] == 255).all()
        assert np.array_equal(H.halves(res, 1, True), 255 - v) and np.array_equal(hz, v.T)


def test_remap_batch_alternates_dark_and_bright_frames_and_holds_every_class():
    names, frames = H.remap_batch(11, 96, 37)
    assert frames.shape == (37, 96, 96) and frames.dtype == np.uint8 and len(names) == 37
    assert set(names[:len(H.REMAP_CLASSES)]) == set(H.REMAP_CLASSES)
    mean = frames.reshape(37, -1).mean(axis=1)
    assert mean[0] < 5 and mean[1] > 250                      # impulses next to holes
    assert np.abs(np.diff(mean)).max() > 240 and frames.min() == 0 and frames.max() == 255
    n2, f2 = H.remap_batch(11, 96, 37)
    assert n2 == names and np.array_equal(f2, frames)
    assert not np.array_equal(frames[2], frames[2 + len(H.REMAP_CLASSES)])  # a later round of a seeded class is a new image


def test_band_pair_sad_bounds():
    """Every |cur - prev| of band_pair(lo) is in [255 - 2 lo, 255]: a 256-pixel SAD with lo = 40 is in [44800, 65280] -- bit 15 set, 16 bits kept
    -- for ANY alignment of the two frames; with lo = 0 it is the 255 * 256 = 65280 that the scans' overflow argument names."""
    cur, prev = H.band_pair(3, (80, 96), 40)
    assert cur.max() == 40 and cur.min() == 0 and prev.min() == 215 and prev.max() == 255
    rng = np.random.default_rng(0)
    for _ in range(200):
        y, x, v, u = (int(t) for t in rng.integers(0, 64, 4))
        sad = int(np.abs(cur[y:y + 16, x:x + 16].astype(np.int32) - prev[v:v + 16, u:u + 16].astype(np.int32)).sum())
        assert 44800 <= sad <= 65280 and sad & 0x8000 and sad < 1 << 16
    c0, p0 = H.band_pair(3, 32, 0)
    assert (c0 == 0).all() and (p0 == 255).all()
    with pytest.raises(ValueError):
        H.band_pair(0, 32, 128)


def test_interpolation_coefficients_are_partitions_of_unity():
    for interp, K in ((2, 4), (4, 8)):
        tab = H.interp_coeffs_f64(interp)
        assert tab.shape == (32, K) and np.allclose(tab.sum(axis=1), 1.0, rtol=0, atol=1e-12)
        assert np.allclose(tab[0], np.eye(K)[K // 2 - 1], rtol=0, atol=1e-15)  # phase 0: the anchor pixel itself
        assert np.allclose(tab[16], tab[16][::-1], rtol=0, atol=1e-12)          # the half-pixel phase is symmetric
    assert np.allclose(H.interp_coeffs_f64(2)[16], [-0.09375, 0.59375, 0.59375, -0.09375])  # A = -0.75 at x = 1/2


def test_bernoulli_noise_places_sums_around_a_16_bit_boundary():
    """Density q = 65536 / (255 * 512) against black: 256-pixel sums stay 16-bit, 512-pixel sums fall on both sides of 2^16."""
    q = 65536.0 / (255.0 * 512)
    a = H.bernoulli_noise(4, (256, 256), q)
    assert np.array_equal(a, H.bernoulli_noise(4, (256, 256), q)) and not np.array_equal(a, H.bernoulli_noise(5, (256, 256), q))
    assert set(np.unique(a)) == {0, 255} and abs((a == 255).mean() - q) < 0.01
    s256 = a.astype(np.int64).reshape(256, 16, 16).sum(axis=2).reshape(-1, 16).sum(axis=1)  # 16 x 16 tiles
    s512 = a.astype(np.int64).reshape(128, 512).sum(axis=1)
    assert s256.max() <= 255 * 256 < 1 << 16 and (s256 >= 1 << 15).any()
    assert (s512 < 1 << 16).sum() >= 16 and (s512 >= 1 << 16).sum() >= 16
    with pytest.raises(ValueError):
        H.bernoulli_noise(0, 8, 1.0)
