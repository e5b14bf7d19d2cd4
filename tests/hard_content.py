"""Hard images for the bit-exact kernels (test helper, numpy only): full-range, saturating and impulse content.

The images of sr_scenes.py and synth.py are low-passed or mid-grey: neighbouring taps differ by a few grey levels, no sum of weighted taps
leaves [0, 255], and no 256-pixel SAD comes near 2^15. Here every generator is seeded and returns uint8 arrays whose extremes are the point:
0 / 255 content drives the remap's sums below 0 and above 255 (both clamps), single impulses turn every tap position and weight into a
destination byte of its own, and `band_pair` puts bit 15 into every 16-bit field of a packed SAD."""
import numpy as np

FOOTPRINT = 8  # the widest interpolation window of the remap (INTER_LANCZOS4: 8 x 8 taps)


def _shape(shape):
    return (shape, shape) if np.isscalar(shape) else tuple(shape)


def binary_noise(seed: int, shape) -> np.ndarray:
    """0 / 255 per pixel, independent, p = 1/2."""
    rng = np.random.default_rng([seed, 1])
    return (rng.integers(0, 2, _shape(shape), dtype=np.uint8) * np.uint8(255)).astype(np.uint8)


def bernoulli_noise(seed: int, shape, q: float) -> np.ndarray:
    """255 with probability q, else 0, independent per pixel. Against a black frame the SAD of n pixels is 255 Binomial(n, q): mean 255 n q,
    sigma 255 sqrt(n q (1 - q)) -- q places the sums of a chosen pixel count around a chosen value (a 16-bit boundary, say)."""
    if not 0.0 < q < 1.0:
        raise ValueError("q must be in (0, 1)")
    rng = np.random.default_rng([seed, 5])
    return np.where(rng.random(_shape(shape)) < q, 255, 0).astype(np.uint8)


def uniform_noise(seed: int, shape) -> np.ndarray:
    """Full-range u8, independent per pixel."""
    return np.random.default_rng([seed, 2]).integers(0, 256, _shape(shape), dtype=np.uint8)


def impulse_positions(seed: int, shape, pitch: int = 12) -> np.ndarray:
    """[n, 2] (y, x) of the impulses of `impulses`: no two of them closer than `pitch` in BOTH axes (so a FOOTPRINT-wide window sees at most
    one as long as pitch > FOOTPRINT). An interior lattice whose phase comes from the seed, kept `pitch` away from the two outermost rows /
    columns; those (0, 1, size - 2, size - 1: the rows and columns that reflect-101 taps land on) carry impulses at alternating lattice
    abscissae -- even lattice indices on the outermost line, odd ones on the second -- and the four corner pixels."""
    h, w = _shape(shape)
    if pitch <= FOOTPRINT:
        raise ValueError(f"pitch {pitch} must exceed the {FOOTPRINT}-tap footprint")
    if min(h, w) < 4 * pitch + 4:
        raise ValueError("image too small for an interior lattice and populated borders")
    rng = np.random.default_rng([seed, 3])
    oy, ox = (int(v) for v in rng.integers(0, pitch, 2))
    ys = np.arange(1 + pitch + oy, h - 2 - pitch + 1, pitch)
    xs = np.arange(1 + pitch + ox, w - 2 - pitch + 1, pitch)
    pts = [(y, x) for y in ys for x in xs]
    for line, odd in ((0, 0), (1, 1), (h - 1, 0), (h - 2, 1)):
        pts += [(line, x) for x in xs[odd::2]]
    for line, odd in ((0, 0), (1, 1), (w - 1, 0), (w - 2, 1)):
        pts += [(y, line) for y in ys[odd::2]]
    pts += [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    return np.array(pts, dtype=np.int64)


def impulses(seed: int, shape, pitch: int = 12) -> np.ndarray:
    """Single 255 pixels on 0 at `impulse_positions`."""
    img = np.zeros(_shape(shape), np.uint8)
    p = impulse_positions(seed, shape, pitch)
    img[p[:, 0], p[:, 1]] = 255
    return img


def holes(seed: int, shape, pitch: int = 12) -> np.ndarray:
    """255 - impulses: single 0 pixels on 255."""
    return (255 - impulses(seed, shape, pitch)).astype(np.uint8)


def checker(shape, p: int = 1, phase: int = 0) -> np.ndarray:
    """Checkerboard of 0 / 255 squares of p x p pixels (p = 1: the Nyquist pattern); phase 1 swaps the colours."""
    h, w = _shape(shape)
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // p) + (xx // p) + phase) & 1) * 255).astype(np.uint8)


def stripes(shape, axis: int = 1, p: int = 1, phase: int = 0) -> np.ndarray:
    """0 / 255 lines of width p: axis 1 = columns alternate (vertical stripes), axis 0 = rows alternate."""
    h, w = _shape(shape)
    yy, xx = np.mgrid[0:h, 0:w]
    return (((((xx if axis == 1 else yy) // p) + phase) & 1) * 255).astype(np.uint8)


def halves(shape, axis: int = 1, white_first: bool = False) -> np.ndarray:
    """Black | white split through the image centre: axis 1 = the edge is the column size // 2 (left black, right white from the centre column
    on), axis 0 = the row size // 2. The log-polar centre (size // 2, size // 2) and its 0 / 90 / 180 / 270 degree rays lie on that edge."""
    h, w = _shape(shape)
    img = np.zeros((h, w), np.uint8)
    if axis == 1:
        img[:, w // 2:] = 255
    else:
        img[h // 2:, :] = 255
    return (255 - img).astype(np.uint8) if white_first else img


def band_pair(seed: int, shape, lo: int = 40):
    """(cur, prev) for the block scans: cur uniform in [0, lo], prev uniform in [255 - lo, 255]. Every |cur - prev| lies in [255 - 2 lo, 255],
    so the SAD of any n pixels lies in [n (255 - 2 lo), 255 n]: with lo = 40 and n = 256 that is [44800, 65280] -- bit 15 set in every 16-bit
    partial sum, none beyond 16 bits -- and the noise keeps the candidates' sums apart."""
    if not 0 <= lo <= 127:
        raise ValueError("lo must be in [0, 127]")
    rng = np.random.default_rng([seed, 4])
    cur = rng.integers(0, lo + 1, _shape(shape), dtype=np.uint8)
    prev = rng.integers(255 - lo, 256, _shape(shape), dtype=np.uint8)
    return cur, prev


REMAP_CLASSES = ("impulses", "holes", "binary_noise", "halves_v_white", "uniform_noise", "checker1", "halves_h", "checker2", "stripes_cols",
                 "halves_v", "stripes_rows", "halves_h_white", "checker1_swapped")


def remap_frame(name: str, seed: int, res: int) -> np.ndarray:
    """One res x res frame of the named class of REMAP_CLASSES."""
    make = {
        "impulses": lambda: impulses(seed, res),
        "holes": lambda: holes(seed, res),
        "binary_noise": lambda: binary_noise(seed, res),
        "uniform_noise": lambda: uniform_noise(seed, res),
        "checker1": lambda: checker(res, 1),
        "checker1_swapped": lambda: checker(res, 1, 1),
        "checker2": lambda: checker(res, 2),
        "stripes_cols": lambda: stripes(res, 1),
        "stripes_rows": lambda: stripes(res, 0),
        "halves_v": lambda: halves(res, 1),
        "halves_h": lambda: halves(res, 0),
        "halves_v_white": lambda: halves(res, 1, True),
        "halves_h_white": lambda: halves(res, 0, True),
    }
    return make[name]()


def remap_batch(seed: int, res: int, n: int):
    """(names, frames[n, res, res]): the classes of REMAP_CLASSES in their order, which alternates black- and white-dominated frames (impulses
    next to holes, the halves next to their complements) so that neighbours in a kernel's image ring differ as much as two frames can; past the
    first round the seeded classes take a new seed and the deterministic ones are complemented on every odd round."""
    names, frames = [], []
    for k in range(n):
        name, rnd = REMAP_CLASSES[k % len(REMAP_CLASSES)], k // len(REMAP_CLASSES)
        f = remap_frame(name, seed + 101 * rnd, res)
        if rnd % 2 == 1 and name not in ("impulses", "holes", "binary_noise", "uniform_noise"):
            f = (255 - f).astype(np.uint8)
        names.append(name if rnd == 0 else f"{name}#{rnd}")
        frames.append(f)
    return names, np.stack(frames)


# ---- an independent float64 restatement of the remap (checks the oracle off smooth content; counts the pixels that really clamp) ----------
def interp_coeffs_f64(interp: int) -> np.ndarray:
    """[32, K] real-valued separable coefficients at the 32 sub-pixel phases f / 32, unrounded float64: interp 2 = bicubic with A = -0.75
    (K = 4, taps at -1 .. 2), interp 4 = Lanczos with a = 4 (K = 8, taps at -3 .. 4: sinc(t) sinc(t / 4), normalised to sum 1)."""
    x = np.arange(32, dtype=np.float64)[:, None] / 32.0
    if interp == 2:
        A = -0.75
        t = np.abs(np.arange(-1, 3, dtype=np.float64)[None, :] - x)  # distance of tap i from the sample
        near = ((A + 2) * t - (A + 3)) * t * t + 1                    # |t| <= 1
        far = ((A * t - 5 * A) * t + 8 * A) * t - 4 * A               # 1 < |t| < 2
        return np.where(t <= 1, near, far)
    if interp == 4:
        t = np.arange(-3, 5, dtype=np.float64)[None, :] - x
        c = np.sinc(t) * np.sinc(t / 4)
        return c / c.sum(axis=1, keepdims=True)
    raise ValueError("interp must be 2 (cubic) or 4 (Lanczos4)")


def logpolar_gather_f64(src: np.ndarray, mapx: np.ndarray, mapy: np.ndarray, interp: int):
    """(value[res, res] float64 unrounded and unclamped, valid[res, res] bool) of cv::remap's fixed-point path restated in real arithmetic:
    map coordinates quantised to 1/32 px (rint(32 m) in float32, >> 5 the anchor, & 31 the phase), separable real coefficients, reflect-101
    taps, a pixel is transparent (valid = False, value 0) when its ANCHOR lies outside the source."""
    src = np.asarray(src)
    h, w = src.shape
    K = 4 if interp == 2 else 8
    half = K // 2 - 1
    tab = interp_coeffs_f64(interp)
    ix = np.rint(np.asarray(mapx, np.float32) * np.float32(32)).astype(np.int64)
    iy = np.rint(np.asarray(mapy, np.float32) * np.float32(32)).astype(np.int64)
    ax, ay, fx, fy = ix >> 5, iy >> 5, ix & 31, iy & 31
    valid = (ax >= 0) & (ax < w) & (ay >= 0) & (ay < h)
    ax, ay = np.clip(ax, 0, w - 1), np.clip(ay, 0, h - 1)

    def reflect(p, n):  # BORDER_REFLECT_101; taps of a valid anchor are at most K / 2 outside, one reflection reaches them
        p = np.abs(p)
        return np.where(p >= n, 2 * n - 2 - p, p)
    s = src.astype(np.float64)
    out = np.zeros(ax.shape, np.float64)
    for k1 in range(K):
        yy = reflect(ay - half + k1, h)
        row = np.zeros(ax.shape, np.float64)
        for k2 in range(K):
            row += tab[fx, k2] * s[yy, reflect(ax - half + k2, w)]
        out += tab[fy, k1] * row
    return np.where(valid, out, 0.0), valid
