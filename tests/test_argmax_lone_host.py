"""CPU test of the short cut behind K1's arg-max barrier at 64 (csrc/pc_argmax.hpp) through tests/cpp/test_argmax_lone, a stand-alone
program built with the address and undefined-behaviour sanitizers: a wave with ONE lane at the maximum folds (wave_best's butterfly,
better()) to that lane's own pair, every lane as the holder, +-0, -inf and 0x7fffffff indices among them; any other count of lanes
keeps the fold. No GPU."""
import os
import subprocess

import pytest


def test_lone_lane_hands_over_what_the_fold_returns():
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(here, "cpp", "test_argmax_lone")
    if not os.path.exists(os.path.join(here, "cpp", "argmax_lone.mk")):
        pytest.skip("tests/cpp/argmax_lone.mk is not in this copy of the tree: sanitizer builds are a CPU-suite job")
    subprocess.check_call(["make", "-C", os.path.join(here, "cpp"), "-s", "-f", "argmax_lone.mk", "test_argmax_lone"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "argmax lone ok" in out.stdout and "lone lane: 9216 waves" in out.stdout, out.stdout
