"""Inputs of the geometry-tail path tests (test_geom_cases_host.py on the CPU, test_gpu_geometry_paths.py on the device): deterministic
getRT scenes chosen for the paths of geom_get_rt_kernel (csrc/mof_geom.hip) that exact, outlier-poor scenes on square grids never reach.

  late       62 % outliers: the accepted RANSAC hypothesis often lies beyond the first round of 64 and the scan ends between rounds; grids
             that are not square, totals of 65 (64 + 1), 255, 256, 260 (4 x 64 + 4, no whole-wave fit) and 1024 (kMaxPoints), each once
             with exact inliers and once with N(0, 0.25 px) on every shift (the refit then has a residual to minimise)
  small_n    0 ... 7 valid patches against thr (n < 4, the n == 4 direct solution, the sampler's `% n` at 5 ... 7), and 63 / 64 / 65
             valid of 65 by position of the NaN patches (the ballot compaction across the 64-lane boundary)
  exits      every status 0 ... 8, the single-solution branch of pick_motion (hover, pure rotation), collinear grids, bad durations,
             thr = -1, nothing valid, no consensus among 1024 points, a camera -> base transform, and 257 patches in one row (the first
             total without the whole-wave fit)
  fit_forms  the same valid points in a 16 x 16 layout (256: homography_fit_wave) and a 16 x 17 layout whose last row is NaN (272: the
             one-lane homography_fit): same a, b and n, so the two device results must be the same bits

A Case carries everything both CPU sides and the device need; nothing here comes from a GPU. Built once per process, read-only."""
import ctypes as C
import functools

import numpy as np

import geom_scenes as S
import oracle_lib as O
from mrs_optic_flow_amd import geometry as G

CAM = (520.0, 518.0, 376.0, 240.0, -0.12, 0.03, 0.0004, -0.0003, -0.002)   # fx, fy, cx, cy, k1, k2, p1, p2, k3
FLAT = CAM[:4] + (0.0,) * 5                                                # the same pinhole without distortion
ORIGIN, STRIDE, PATCH = (1, 2), (30, 40), 32
HEIGHT, DT, ULX = 2.5, 0.02, 0.0
PAIRS = 32                                                                 # per late geometry
NOISE_PX = 0.25
# (grid_x, grid_y, noise seed): 65 = 64 + 1 both ways round, 256, 255, 1024 = kMaxPoints, 260 = 4 x 64 + 4 (beyond kWaveFitPoints).
# Scene seed: grid_x * 100 + grid_y. A minimal model fitted to four noisy points can miss a far inlier by more than the threshold, and the
# mask is that model's: the noise seed of each grid is the first (counting from 50000 + scene seed) at which all 32 pairs keep the planted
# set in the CPU oracle, so that the noisy scenes can be held to it like the exact ones.
LATE_GRIDS = ((13, 5, 0), (5, 13, 0), (16, 16, 1), (17, 15, 0), (32, 32, 4), (20, 13, 0))
IDENT_Q = (0.0, 0.0, 0.0, 1.0)


class Case:
    """One frame pair. layout = (grid_x, grid_y, origin_x, origin_y, stride_x, stride_y, patch); params = (height, dt, ul_corner_x,
    ang_rate_q, c2b_q, c2b_t); planted = the consensus set a planted scene must recover (bool [total]) or None."""

    def __init__(self, family, name, shifts, layout, cam, thr, height=HEIGHT, dt=DT, ang_q=IDENT_Q, c2b_q=IDENT_Q, c2b_t=(0.0, 0.0, 0.0),
                 planted=None, group=None):
        self.family, self.name, self.layout, self.cam, self.thr = family, name, tuple(layout), tuple(cam), int(thr)
        self.shifts = np.ascontiguousarray(shifts, dtype=np.float64)
        assert self.shifts.shape == (layout[0] * layout[1], 2)
        self.params = (float(height), float(dt), ULX, tuple(float(v) for v in ang_q), tuple(float(v) for v in c2b_q),
                       tuple(float(v) for v in c2b_t))
        self.planted = planted
        self.group = group                      # late: the geometry's name (coverage is counted per geometry)
        self.shifts.setflags(write=False)
        if planted is not None:
            planted.setflags(write=False)

    @property
    def total(self):
        return self.layout[0] * self.layout[1]

    @property
    def valid(self):
        return np.isfinite(self.shifts).all(axis=1)

    @property
    def key(self):
        """what one device launch shares"""
        return self.layout, self.cam, self.thr

    def _structs(self, lay, cam, par):
        h, dt, ulx, aq, cq, ct = self.params
        return lay(*self.layout), cam(*self.cam), par(h, dt, ulx, (C.c_double * 4)(*aq), (C.c_double * 4)(*cq), (C.c_double * 3)(*ct))

    def lib_args(self):
        return self._structs(G.Layout, G.Camera, G.RtParams)

    def oracle_args(self):
        return self._structs(O.GeomLayout, O.GeomCamera, O.GeomRtParams)

    def param_row(self):
        """the 14 doubles of one RtParams row of the device parameter array"""
        h, dt, ulx, aq, cq, ct = self.params
        return np.array((h, dt, ulx) + aq + cq + ct)

    def points(self):
        """the normalised pairs (a, b) the tail forms from the valid patches, in patch order (for the scan probe)"""
        gx, gy, ox, oy, sx, sy, patch = self.layout
        c = S.patch_centres(gx, gy, (ox, oy), (sx, sy), patch)[self.valid]
        cam = G.Camera(*self.cam)
        return G.undistort_points(cam, ULX, c), G.undistort_points(cam, ULX, c + self.shifts[self.valid])


def host(case):
    """the library's host form -> (status, rot, tran, mask, H)"""
    lay, cam, par = case.lib_args()
    return G.get_rt(case.shifts, lay, cam, par, case.thr)


def oracle(case):
    lay, cam, par = case.oracle_args()
    return O.geom_get_rt(case.shifts, lay, cam, par, case.thr)


def _layout(gx, gy, stride=STRIDE):
    return (gx, gy, ORIGIN[0], ORIGIN[1], stride[0], stride[1], PATCH)


def motion(rng, angle=None, translate=True):
    """a small rigid motion above the ground plane: (H on normalised coordinates, the IMU quaternion the node would form)"""
    axis = rng.normal(size=3)
    angle = rng.uniform(0.002, 0.02) if angle is None else angle
    t = rng.normal(0, 0.02, 3) if translate else np.zeros(3)
    H = S.plane_homography(S.rot_axis_angle(axis, angle), t, np.array([0.0, 0.0, 1.0]), HEIGHT)
    rate = axis / np.linalg.norm(axis) * angle / DT
    return H, tuple(O.geom_quat_from_rpy(*(-rate)))


def shifts_of(layout, cam, H):
    gx, gy, ox, oy, sx, sy, patch = layout
    return S.shifts_for_motion(cam, ULX, S.patch_centres(gx, gy, (ox, oy), (sx, sy), patch), H)


def planted_scene(rng, layout, cam, outliers, nans):
    """test_geometry._rt_scene's construction: exact shifts of one motion, `outliers` patches thrown 12 ... 40 px off (the RANSAC threshold
    is 0.01 * f = 5 px), `nans` patches invalid. -> shifts, IMU quaternion, planted consensus set"""
    H, q = motion(rng)
    sh = shifts_of(layout, cam, H)
    total = len(sh)
    idx = rng.permutation(total)
    bad, nan = idx[:outliers], idx[outliers:outliers + nans]
    sh[bad] += rng.choice([-1.0, 1.0], (outliers, 2)) * rng.uniform(12, 40, (outliers, 2))
    sh[nan] = np.nan
    planted = np.ones(total, bool)
    planted[bad] = planted[nan] = False
    return sh, q, planted


def _late_geometry(gx, gy, noise_seed=None, outlier_share=0.62, pairs=PAIRS, family="late", layout=None, tag=None, stride=STRIDE):
    layout = layout or _layout(gx, gy, stride)
    total = gx * gy
    rng = np.random.default_rng(gx * 100 + gy)
    noisy = noise_seed is not None
    noise = np.random.default_rng(gx * 100 + gy + 50000 + (noise_seed or 0))
    group = tag or f"{family} {gx}x{gy} {'noisy' if noisy else 'exact'}"
    out = []
    for k in range(pairs):
        sh, q, planted = planted_scene(rng, _layout(gx, gy, stride), CAM, int(outlier_share * total), (k % 3) * total // 12)
        if noisy:
            sh = sh + noise.normal(0, NOISE_PX, sh.shape)
        if layout[0] * layout[1] > total:       # fit_forms: the same patches, then rows of invalid ones
            pad = layout[0] * layout[1] - total
            sh, planted = np.concatenate([sh, np.full((pad, 2), np.nan)]), np.concatenate([planted, np.zeros(pad, bool)])
        out.append(Case(family, f"{group} #{k}", sh, layout, CAM, 8, ang_q=q, planted=planted, group=group))
    return out


@functools.lru_cache(maxsize=None)
def late():
    return tuple(c for gx, gy, seed in LATE_GRIDS for noise_seed in (None, seed) for c in _late_geometry(gx, gy, noise_seed))


def _keep(sh, keep):
    out = np.full_like(sh, np.nan)
    out[list(keep)] = sh[list(keep)]
    return out


SMALL_GRID = (7, 5)
# valid patches of the 7 x 5 grid, nested: the corners first (no three on a line), the last patch (34) always among them
SMALL_VALID = (0, 34, 6, 28, 17, 3, 31)
SMALL_ROWS = ((0, 0), (3, 0), (3, 3), (4, 4), (4, 0), (5, 4), (5, 5), (4, 5), (6, 4), (7, 7))    # (valid, thr)
# NaN patches of the 13 x 5 grid (total 65): valid counts 65, 64 (first / last / middle missing), 63, and only the last 21 valid
EDGE_NANS = {"65 valid": (), "64 valid, last missing": (64,), "64 valid, first missing": (0,), "64 valid, 31 missing": (31,),
             "63 valid, 0 and 64 missing": (0, 64), "63 valid, 63 and 64 missing": (63, 64), "63 valid, 62 and 63 missing": (62, 63),
             "21 valid, the last ones": tuple(range(44))}


@functools.lru_cache(maxsize=None)
def small_n():
    rng = np.random.default_rng(705)
    lay = _layout(*SMALL_GRID)
    out = []
    for valid, thr in SMALL_ROWS:
        H, q = motion(rng)
        sh = _keep(shifts_of(lay, CAM, H), SMALL_VALID[:valid])
        out.append(Case("small_n", f"small_n {valid} valid thr {thr}", sh, lay, CAM, thr, ang_q=q, planted=np.isfinite(sh[:, 0])))
    lay = _layout(13, 5)
    for name, nans in EDGE_NANS.items():
        H, q = motion(rng)
        sh = shifts_of(lay, CAM, H)
        sh[list(nans)] = np.nan
        out.append(Case("small_n", f"small_n 13x5 {name}", sh, lay, CAM, 8, ang_q=q, planted=np.isfinite(sh[:, 0])))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exits():
    rng = np.random.default_rng(75)
    lay = _layout(*SMALL_GRID)
    nan_q = (np.nan, 0.0, 0.0, 1.0)
    out = []

    def add(name, sh, layout=lay, cam=CAM, thr=8, **kw):
        out.append(Case("exits", "exits " + name, sh, layout, cam, thr, **kw))

    H, q = motion(rng)
    general = shifts_of(lay, CAM, H)
    Hr, qr = motion(rng, translate=False)
    rotation = shifts_of(lay, CAM, Hr)
    add("general motion", general, ang_q=q)
    add("zero shifts (hover)", np.zeros_like(general))                       # H = I: the single-solution branch, identity / zero out
    add("pure rotation", rotation, ang_q=qr)                                 # single solution, accepted
    add("pure rotation, NaN IMU", rotation, ang_q=nan_q)                     # 5: single solution, none accepted
    add("pure rotation, height inf", rotation, ang_q=qr, height=np.inf)      # 6: 0 * inf in the translation
    add("general motion, NaN IMU", general, ang_q=nan_q)                     # 7: four solutions, none accepted
    add("IMU disagrees", general, ang_q=tuple(O.geom_quat_from_rpy(0, 0, 3.0)))   # 4
    for name, dt in (("0", 0.0), ("-0", -0.0), ("NaN", np.nan)):
        add(f"dt {name}", general, ang_q=q, dt=dt)                           # 1
    add("thr -1", general, ang_q=q, thr=-1)                                  # 2: uint(-1) is never reached
    add("all NaN", np.full_like(general, np.nan), ang_q=q)                   # 2
    add("all NaN thr 0", np.full_like(general, np.nan), ang_q=q, thr=0)      # 8
    add("cam -> base transform", general, ang_q=q, c2b_q=tuple(O.geom_quat_from_rpy(0.1, -0.2, 1.5)), c2b_t=(0.05, 0.0, -0.1))
    # collinear centres: exactly so under the pinhole (no minimal set is non-degenerate), only nearly so under the distortion
    for gx, gy in ((12, 1), (1, 12)):
        line = _layout(gx, gy)
        H, q = motion(rng)
        for cam, cname in ((FLAT, "flat"), (CAM, "distorted")):
            for thr in (0, 8):
                add(f"collinear {gx}x{gy} {cname} thr {thr}", shifts_of(line, cam, H), layout=line, cam=cam, thr=thr, ang_q=q)
    # 257 = kWaveFitPoints + 1 is a prime: one row, which the distortion bends off a straight line by 3 x the RANSAC threshold
    out.extend(_late_geometry(257, 1, pairs=4, family="exits", stride=(2, 0), tag="exits 257x1"))
    big = _layout(32, 32)
    add("no consensus 32x32", rng.uniform(-CAM[0], CAM[0], (1024, 2)), layout=big, ang_q=q)   # 3 after all 2000 hypotheses
    return tuple(out)


FIT_LAYOUTS = (_layout(16, 16), _layout(16, 17))    # 256 patches: whole-wave refit; 272, the last row NaN: one-lane refit
FIT_PAIRS = 8
FIT_SHARES = ((0.38, 1), (0.9, 5))                 # (inlier share, noise seed as in LATE_GRIDS)


@functools.lru_cache(maxsize=None)
def fit_forms():
    """-> (cases in the 256 layout, the same scenes in the 272 layout), index by index"""
    both = []
    for layout in FIT_LAYOUTS:
        cs = []
        for share, seed in FIT_SHARES:
            for noise_seed in (None, seed):
                cs += _late_geometry(16, 16, noise_seed, outlier_share=round(1 - share, 2), pairs=FIT_PAIRS, family="fit_forms", layout=layout,
                                     tag=f"fit_forms {layout[0] * layout[1]} share {share} {'exact' if noise_seed is None else 'noisy'}")
        both.append(tuple(cs))
    return tuple(both)


@functools.lru_cache(maxsize=None)
def everything():
    return late() + small_n() + exits() + fit_forms()[0] + fit_forms()[1]


def batches(cases):
    """cases grouped by what one device launch shares: {(layout, cam, thr): [case, ...]} in first-seen order"""
    out = {}
    for c in cases:
        out.setdefault(c.key, []).append(c)
    return out


@functools.lru_cache(maxsize=None)
def references():
    """{case name: (host form's result, oracle's result)}: computed once, shared by the CPU and the GPU tests"""
    return {c.name: (host(c), oracle(c)) for c in everything()}
