"""One small case per route class of the FFT engine's default route table (tests/golden/fft_route_table.txt): inputs and the CPU oracles'
references of test_gpu_fft_route_classes.py, and what test_route_cases_host.py checks about them without a GPU.

A route class = everything the table records about a (peak model, patch size) but the sizes themselves: the family, whether pair
launches run on the half tile, the video form, and the three flags of the large pipeline. The default table holds 16 of them; the
cases below stand at each class's smallest size (under cv::phaseCorrelate's model the first PADDED planned size, 37 -> 40, stands for
the planned class and 162 for the half-tile class without a video form; under the OpenCL model 48 for the planned class).

A case: frames of one row of two patches (origin 0, stride = patch size), three frames of the (1 6 1)-blurred texture
(mrs_optic_flow_amd/synth.py, blur="mild") displaced by known integers, so that the pair entry sees the pairs (1, 0) and (2, 1) and the
video entry the three frames. Built once per process, shared, read-only.
"""
import functools
import os

import numpy as np

import oracle_lib as O
from mrs_optic_flow_amd import synth

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fft_route_table.txt")
PEAK_OPENCV, PEAK_OCL = 0, 1  # include/mof.h
# (peak model, patch size) -> the class it stands for, in the words of the table's columns:
# (family, pairs on the half tile, video form, large_tuned, odd_tail, large_video)
CASES = {
    (PEAK_OPENCV, 37): ("PLANNED", False, "PAIRS", 0, 0, 0),
    (PEAK_OPENCV, 32): ("TUNED", False, "PAIRS", 0, 0, 0),
    (PEAK_OPENCV, 49): ("PLANNED", False, "HALF_SEQ", 0, 0, 0),
    (PEAK_OPENCV, 60): ("PLANNED", True, "HALF_SEQ", 0, 0, 0),
    (PEAK_OPENCV, 64): ("TUNED", False, "SEQ", 0, 0, 0),
    (PEAK_OPENCV, 120): ("TUNED", True, "HALF_SEQ", 0, 0, 0),
    (PEAK_OPENCV, 128): ("TUNED", False, "HALF_SEQ", 0, 0, 0),
    (PEAK_OPENCV, 136): ("LARGE", True, "HALF_SEQ", 0, 0, 0),
    (PEAK_OPENCV, 162): ("LARGE", True, "PAIRS", 0, 0, 0),
    (PEAK_OPENCV, 193): ("LARGE", False, "PAIRS", 1, 0, 1),
    (PEAK_OPENCV, 244): ("LARGE", False, "PAIRS", 1, 1, 1),
    (PEAK_OCL, 48): ("PLANNED", False, "PAIRS", 0, 0, 0),
    (PEAK_OCL, 32): ("TUNED", False, "PAIRS", 0, 0, 0),
    (PEAK_OCL, 64): ("TUNED", False, "SEQ", 0, 0, 0),
    (PEAK_OCL, 128): ("TUNED", False, "SEQ_HALF", 0, 0, 0),
    (PEAK_OCL, 144): ("LARGE", False, "PAIRS", 0, 0, 0),
}
# frame t shows the texture displaced by OFFSETS[t]: pair (1, 0) moves by (3, -2), pair (2, 1) by (-5, 3)
OFFSETS = ((0, 0), (3, -2), (-2, 1))
# The texture index of a case is SEED + its patch size. Chosen on the CPU, from the oracles and the pixels alone, so that
# test_route_cases_host.py holds: of the seeds 1 .. 39 only 17, 26 and 31 keep the two oracles within 2e-5 px of each other on all 64
# patches (the OpenCL model's cases at 128 and 144 decide: 2.1e-5 .. 5.7e-5 px under the other seeds); 31 has the largest margin, 1.4e-5 px.
SEED = 31
SEARCH_RADIUS = 55


@functools.lru_cache(maxsize=None)
def default_table():
    """{(peak model, patch size): None (unsupported) or (family, m, half_m, video, video_m, large_tuned, odd_tail, large_video)} of the
    table's `default` section"""
    rows, inside = {}, False
    for line in open(TABLE):
        if line.startswith("#"):
            continue
        if line.startswith("knobs "):
            inside = line.split()[1] == "default"
            continue
        if inside:
            f = line.split()
            rows[(int(f[0]), int(f[1]))] = None if f[2] == "unsupported" else (f[2], int(f[3]), int(f[4]), f[5], int(f[6]), int(f[7]), int(f[8]), int(f[9]))
    return rows


def route_class(row):
    return None if row is None else (row[0], row[2] > 0, row[3], row[5], row[6], row[7])


def variant(row):
    """mof_fft_kernel_variant of a table row"""
    return "planned-half" if row[2] > 0 else {"TUNED": "stockham", "PLANNED": "planned", "LARGE": "planned-large"}[row[0]]


class Case:
    def __init__(self, model, n):
        self.model, self.n = model, n
        self.shape = (n, 2 * n)  # one row of two patches
        self.frames = np.stack([synth.pair_np(SEED + n, n, 2 * n, dx, dy, blur="mild")[0] for dx, dy in OFFSETS])
        self.lay = O.fft_layout(2 * n, n, n, 2, 1)
        self.want64, self.want32 = (np.stack([self._oracle(k, prec) for k in range(2)]) for prec in (64, 32))  # [pair, patch, xy]
        for a in (self.frames, self.want64, self.want32):
            a.setflags(write=False)

    def _oracle(self, k, precision):
        cur, prev = self.frames[k + 1], self.frames[k]
        if self.model == PEAK_OCL:
            return O.fft_process_ocl(cur, prev, self.lay, SEARCH_RADIUS, precision)[0]
        return O.fft_process(cur, prev, self.lay, precision)[0]

    def patch_pixels(self, k, p):
        """(cur patch, prev patch) of patch p of pair k"""
        n = self.n
        return self.frames[k + 1][:, p * n:(p + 1) * n], self.frames[k][:, p * n:(p + 1) * n]


@functools.lru_cache(maxsize=None)
def case(model, n):
    return Case(model, n)
