"""GPU tests of the per-patch correlation quality on the kernel forms a knob selects and on forced pass / run / chunk boundaries.

The MOF_FFT_* knobs are read once per process (mof_capi.hip fft_knobs, behind fft_route; host_pipe.hpp), so every form runs
in ONE child process with the environment set -- the convention of test_gpu_kernel_forms.py and test_gpu_generic.py. The child runs
the route tests of test_gpu_fft_quality.py (the f64 oracle at 360 d, quality_cases.py; the shifts' bits with and without the quality
output), which take their batches and the kernel_variant or bit relation they expect from MOF_QUALITY_PAIRS / _LONG_RANGE / _VIDEOS:
the existing tests' asserts of the DEFAULT variants stay as they are and are not selected here. Children run one after another, each
under its own time limit, pytest -x; a child that ends on a signal or a non-zero status fails its parent test, which shows the tail
of the child's output. The parent prints every line the child measured (run with -s).

Evidence that a knob took effect is asserted wherever the library exposes the route: kernel_variant (checked in the child against the
parametrisation and again here in the child's output), and the video entry taking the pair entry's bits where it has bits of its own by
default (test_sequence_runs asserts either). Where nothing exposes the route the docstring says so."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGET = os.path.join(ROOT, "tests", "test_gpu_fft_quality.py")
FORMS_TARGET = os.path.join(ROOT, "tests", "test_gpu_fft_launch_forms.py")


def _cases(pairs):
    return ",".join(f"{name}={what}" for name, what in pairs)


_DIED = []  # a child that ended on a signal or at its time limit: no later test of this module starts another on the same card


def _child(env, select, pairs=(), long_range=(), videos=(), forms=(), timeout=600):
    """One child: the selected route tests under `env`. Returns its stdout after the status checks; every expected route line
    ('route <name>: kernel_variant <variant>', printed by the child before it asserts) must be there.
    `forms`: (case, kernel_variant) of tests/launch_form_cases.py -- the front-end forms (BGR8, the OpenCL model, the long-range mode)
    of the kernels the knob selects, held to the oracle by test_gpu_fft_launch_forms.py::test_launch_form_on_its_route in the same
    child ('form <name>: kernel_variant <variant>')."""
    if _DIED:
        pytest.fail(f"not started: an earlier child of this module died ({_DIED[0]}); find its cause first")
    e = dict(os.environ, **env)
    e.update(MOF_QUALITY_PAIRS=_cases(pairs), MOF_QUALITY_LONG_RANGE=_cases(long_range), MOF_QUALITY_VIDEOS=_cases(videos))
    targets = [TARGET]
    if forms:
        e.update(MOF_LAUNCH_FORM_CASES=_cases(forms))
        targets.append(FORMS_TARGET)
        select = f"({select}) or test_launch_form_on_its_route"
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", *targets, "-m", "gpu", "-x", "-q", "-s", "-k", select, "-p", "no:cacheprovider"],
                           capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=e)
    except subprocess.TimeoutExpired:
        _DIED.append(f"{env}: no end within {timeout} s")
        raise
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        _DIED.append(f"{env}: status {r.returncode}")
    for line in r.stdout.splitlines():
        if "bar " in line or "route " in line or "form " in line or " passed" in line:
            print(f"[{' '.join(f'{k}={v}' for k, v in env.items())}] {line}")
    assert r.returncode == 0 and " passed" in r.stdout and " skipped" not in r.stdout and " deselected" in r.stdout, \
        (env, r.returncode, r.stdout[-3000:], r.stderr[-1500:])
    for name, variant in list(pairs) + list(long_range):
        assert f"route {name}: kernel_variant {variant}" in r.stdout, (env, name, variant, r.stdout[-3000:])
    for name, variant in forms:
        assert f"form {name}: kernel_variant {variant}" in r.stdout, (env, name, variant, r.stdout[-3000:])
    for name, bits in videos:
        m = re.search(rf"route {re.escape(name)}: kernel_variant \S+, video entry == pair entry bits: (True|False)", r.stdout)
        assert m and m.group(1) == str(bits == "pair"), (env, name, bits, r.stdout[-3000:])
    return r.stdout


def _forms(variant, *names):
    return [(name, variant) for name in names]


ROUTES = "test_pair_entry_on_its_route or test_sequence_runs"
CONSTANTS = "test_constant_and_zero"  # (patches, frames in a video: they assert no variant, they print it)


def test_the_older_forms(gpu):
    """MOF_FFT_HALF=0, MOF_FFT_LARGE_TUNED=0, MOF_PLANNED_STATIC=0, MOF_FFT_SEQ_PAIRS=1 (they act on different sizes): 142 -> 144 and
    120 without the half tile (the large pipeline; the tuned 120 kernel of pc_kernel_mixed.hip), 200 and 196 -> 200 on L5 - L8, 54 and
    62 on the run-time plan, every video on the pair form; the constant and zero patches of every family on these forms.
    Evidence: kernel_variant at 120 and 142 (planned-half by default); the video entry has the pair entry's bits at 64 and 128, where
    the sequence kernels are kernels of their own (test_sequence_runs asserts by default that it has not). Nothing exposes
    MOF_FFT_LARGE_TUNED or MOF_PLANNED_STATIC: kernel_variant is 'planned-large' / 'planned' either way."""
    _child({"MOF_FFT_HALF": "0", "MOF_FFT_LARGE_TUNED": "0", "MOF_PLANNED_STATIC": "0", "MOF_FFT_SEQ_PAIRS": "1"},
           f"{ROUTES} or {CONSTANTS}",
           pairs=[("circular-120", "stockham"), ("padded-142", "planned-large"), ("circular-200", "planned-large"),
                  ("padded-196", "planned-large"), ("passes-200", "planned-large"), ("circular-54", "planned"), ("padded-62", "planned")],
           videos=[("long-video-64", "pair"), ("long-video-120", "pair"), ("long-video-128", "pair"), ("long-video-200", "pair")],
           forms=_forms("planned", "planned-11-gray-cv", "planned-11-bgr-cv", "planned-11-lr-cv", "planned-20-gray-cv", "planned-20-bgr-cv",
                        "planned-20-lr-cv", "planned-20-gray-ocl", "planned-20-bgr-ocl", "planned-20-lr-ocl", "planned-74-gray-cv",
                        "planned-74-bgr-cv", "planned-74-lr-cv", "video-50-bgr-cv")
           + _forms("stockham", "k1-120-gray-cv", "k1-120-bgr-cv", "k1-120-lr-cv", "video-64-bgr-cv", "video-64-gray-ocl", "video-64-bgr-ocl",
                    "video-128-bgr-cv", "video-128-bgr-ocl", "video-120-bgr-cv")
           + _forms("planned-large", "half-144-gray", "half-144-bgr"))


def test_the_half_tile_everywhere(gpu):
    """MOF_FFT_HALF=1: 64 and 128 through the half-tile kernel, pairs (the tiled 128 frames: 512 patches) and its sequence form on the
    long videos (fft_route takes the half tile's video form before it looks at MOF_FFT_SEQ_HALF128, so that one has a child of
    its own); the constant and zero patches. Evidence: kernel_variant 'planned-half' at 64 and 128 ('stockham' by default); the
    video entry has the pair entry's bits at 64 and 128 (the half tile's two forms share their arithmetic, as at 120 by default).
    The front-end forms: gray and BGR8 pairs and videos at 64 and 128 on the half tile; the OpenCL model, which the half tile does
    not have, stays on K1 ('stockham'), and so does the long-range mode (kernel_variant names the full-resolution route)."""
    _child({"MOF_FFT_HALF": "1"}, f"{ROUTES} or {CONSTANTS}",
           pairs=[("circular-64", "planned-half"), ("crops-64", "planned-half"), ("grid-64", "planned-half"),
                  ("circular-128", "planned-half"), ("tiled-128", "planned-half")],
           videos=[("long-video-64", "pair"), ("long-video-128", "pair"), ("video-64", "pair"), ("video-128", "pair")],
           forms=_forms("planned-half", "k1-64-gray-cv", "k1-64-bgr-cv", "k1-128-gray-cv", "k1-128-bgr-cv", "video-64-gray-cv", "video-64-bgr-cv",
                        "video-128-bgr-cv", "k1-64-lr-cv")
           + _forms("stockham", "k1-64-bgr-ocl", "k1-128-bgr-ocl"))


def test_the_older_half_tile_sequence_kernels(gpu):
    """MOF_FFT_SEQ_HALF128=1, MOF_FFT_SEQ_RUN=3: pc_seq_half.hip's sequence kernel at 128, the one size it serves, in runs of three (it
    takes 16 by default, which the 10 pairs would not fill: the kernel must see a second run). Nothing exposes the route: kernel_variant
    names the pair kernel, 'stockham' either way, and the video entry has not the pair entry's bits with or without the knob. The
    front-end forms: gray and BGR8 videos under both peak models -- the four instantiations of pc_seq_half_kernel."""
    _child({"MOF_FFT_SEQ_HALF128": "1", "MOF_FFT_SEQ_RUN": "3"}, "test_sequence_runs",
           videos=[("long-video-128", "own"), ("video-128", "own")],
           forms=_forms("stockham", *(f"video-128-{f}-{m}" for f in ("gray", "bgr") for m in ("cv", "ocl"))))


def test_forced_planned_kernel(gpu):
    """MOF_FFT_FORCE_PLANNED=1: 32, 64, 120 and 128 through the planned kernel (pc_kernel_generic.hip), also under the OpenCL model at
    64, the long-range mode at 120 and the videos (the pair form); the constant and zero patches. Evidence: kernel_variant 'planned'
    ('stockham' / 'planned-half' by default); the video entry has the pair entry's bits at 64 and 128."""
    _child({"MOF_FFT_FORCE_PLANNED": "1"}, f"{ROUTES} or test_long_range_beyond_32 or {CONSTANTS}",
           pairs=[("circular-32", "planned"), ("circular-64", "planned"), ("grid-64", "planned"), ("circular-120", "planned"),
                  ("circular-128", "planned"), ("ocl-64", "planned")],
           long_range=[("long-range-120", "planned")],
           videos=[("long-video-64", "pair"), ("long-video-120", "pair"), ("long-video-128", "pair")])


def test_forced_large_pipeline(gpu):
    """MOF_FFT_FORCE_LARGE=1: 64, 120 and 142 -> 144 through the pipeline in device memory (L5 - L8: below 200 there are no tuned
    transforms), the OpenCL model at 144 in one and in several pairs per frame; fft_route sends the OpenCL model at the planned sizes
    to the planned kernel, so 64 and 60 run that. The constant and zero patches at 64, 120 and 144 (the counted bar of the large
    pipeline). Evidence: kernel_variant."""
    _child({"MOF_FFT_FORCE_LARGE": "1"}, f"{ROUTES} or (test_constant_and_zero_patches and (64 or 120 or 144))",
           pairs=[("circular-64", "planned-large"), ("grid-64", "planned-large"), ("circular-120", "planned-large"),
                  ("padded-142", "planned-large"), ("ocl-144", "planned-large"), ("ocl-passes-144", "planned-large"),
                  ("ocl-64", "planned"), ("ocl-60", "planned")],
           videos=[("long-video-64", "pair"), ("long-video-120", "pair")])


def test_videos_on_the_pair_form_of_their_family(gpu):
    """MOF_FFT_LARGE_VIDEO=0, MOF_FFT_HALF_SEQ=0: the videos at 200 and 120 as pairs of consecutive frames (every frame transformed
    twice). The video entry must keep the pair entry's bits; it has them by default too at these sizes, so nothing exposes the route."""
    _child({"MOF_FFT_LARGE_VIDEO": "0", "MOF_FFT_HALF_SEQ": "0"}, "test_sequence_runs",
           videos=[("long-video-200", "pair"), ("long-video-120", "pair"), ("video-200", "pair"), ("video-120", "pair")])


def test_forced_pass_run_and_chunk_boundaries(gpu):
    """MOF_FFT_LARGE_PASS=3, MOF_FFT_SEQ_RUN=3, MOF_HOST_CHUNK=2: the 10 pairs at 200 and the 7 under the OpenCL model at 144 take four
    and three passes of the scratch (launch_large's k0 offset), the video at 200 passes of its video form, the long videos at 64, 120
    and 128 runs of three with a ragged last one (the run walkers' p0 offset), the 7 pairs of 3 x 2 patches four host chunks as pairs
    and as a video (the HostPipe's second output). The boundaries are not exposed; what is asserted is that the quality stays the
    oracle's and, for the host entry, the device entry's bits."""
    _child({"MOF_FFT_LARGE_PASS": "3", "MOF_FFT_SEQ_RUN": "3", "MOF_HOST_CHUNK": "2"}, f"{ROUTES} or test_host_entry_chunks or test_grid_order_3x2",
           pairs=[("passes-200", "planned-large"), ("ocl-passes-144", "planned-large"), ("padded-246", "planned-large")],
           videos=[("long-video-64", "own"), ("long-video-120", "pair"), ("long-video-128", "own"), ("long-video-200", "pair")])

