"""CPU test of the pairing of the three fp64 sums in K1's finish kernel (csrc/pc_finish_tree.hpp) through tests/cpp/test_finish_tree: on
random leaves, leaves of +0.0 and -0.0, all-zero leaves and single-leaf windows the helper returns, bit for bit, what lane 0 holds after
a plain simulation of the 64 lanes running a[l] += a[l ^ OFF] for OFF = 32 .. 1. No GPU."""
import os
import subprocess


def test_tree_is_lane_zero_of_the_wave_sum():
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(here, "cpp", "test_finish_tree")
    # (built by __graft_entry__.build(); rebuilt here when the header or the driver is newer)
    subprocess.check_call(["make", "-C", os.path.join(here, "cpp"), "-s", "-f", "finish_tree.mk", "test_finish_tree"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "finish tree ok" in out.stdout
