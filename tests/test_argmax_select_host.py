"""CPU test of the selection rule of K1's value-first arg-max (csrc/pc_argmax.hpp) through tests/cpp/test_argmax_select: on arrays of
4 x 64 x 16 candidates with planted ties, +0 against -0, -inf and NaN, the value-first flow returns the (value bits, index) of the
sequential better() fold and of the pair-fold flow it replaces. No GPU."""
import os
import subprocess


def test_value_first_selects_what_the_pair_fold_selects():
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(here, "cpp", "test_argmax_select")
    # (built by __graft_entry__.build(); rebuilt here when the header or the driver is newer)
    subprocess.check_call(["make", "-C", os.path.join(here, "cpp"), "-s", "-f", "argmax_select.mk", "test_argmax_select"])
    out = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "argmax select ok" in out.stdout
