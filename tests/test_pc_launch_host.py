"""CPU test of the launch layer's host logic (csrc/pc_launch.hpp) through tests/cpp/test_pc_launch: the form dispatch maps every
(downscale, channels, peak_model) of a form set to its compile-time constants and refuses everything else, the enumeration visits
exactly the forms the dispatch can return, the 65535-pair split advances cur / prev / out / quality / total as the launchers need
(batches of 0 .. 2 x 65535 + 1 pairs), and the CU count falls back to 256 where no device answers."""
import os
import subprocess


def test_dispatch_enumeration_and_pair_split():
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(here, "cpp", "test_pc_launch")
    # (always through make: its prerequisites decide whether a binary left from an older pc_launch.hpp is rebuilt)
    subprocess.check_call(["make", "-C", os.path.join(here, "cpp"), "-s", "test_pc_launch"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pc_launch: 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
