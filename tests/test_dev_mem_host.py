"""CPU test of the engines' resource owners (csrc/dev_mem.hpp) and the one scratch-growth guard (csrc/capi_graph.hpp) through
tests/cpp/test_dev_mem: the owners are move-only, a move leaves its source empty, reset() and the destructor do nothing on an empty
owner; where no device answers alloc / create return the HIP error, leave the owner empty and the live-buffer count at zero; the guard
refuses a pinned engine with MOF_ERR_BUSY and a capturing stream with MOF_ERR_BAD_ARG, asks for the fallback size and returns the
failure's code when the re-allocation fails, and does not call the allocator when the size already fits."""
import os
import subprocess


def test_owners_and_growth_guard():
    here = os.path.dirname(os.path.abspath(__file__))
    binary = os.path.join(here, "cpp", "test_dev_mem")
    # (always through make: its prerequisites decide whether a binary left from an older header is rebuilt)
    subprocess.check_call(["make", "-C", os.path.join(here, "cpp"), "-s", "test_dev_mem"])
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "dev_mem: 0 failures" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
