import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # built artefacts are git-ignored: a fresh checkout builds them once (hipcc cross-compiles gfx950 without a GPU)
    need = [os.path.join(ROOT, "mrs_optic_flow_amd", "libmof_hip.so"), os.path.join(ROOT, "oracle", "liboracle.so"),
            os.path.join(ROOT, "tests", "cpp", "test_processors")]
    if os.path.exists("/root/reference/include/OpticFlowCalc.h"):  # the adapter compile test needs the reference's header
        need.append(os.path.join(ROOT, "oracle", "_ref", "test_adapter"))
    if not all(os.path.exists(p) for p in need):
        import __graft_entry__

        __graft_entry__.build()


@pytest.fixture(scope="session")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible (there is no CPU fallback)")
    return torch.device("cuda:0")


def pytest_sessionfinish(session, exitstatus):
    """Every patch of this session that left the plain 1e-4 px bar (tests/tolerances.py): mechanism, the independent f32 libraries'
    distances, the bar, the kernel's distances -> one JSON file; and the session's bounds on how many there may be, over EVERY module's
    records (a violation turns a green session red)."""
    try:
        import json

        import tolerances
    except Exception:
        return
    if not tolerances.RECORDS:
        return
    bad = tolerances.violations()
    path = os.environ.get("MOF_F32_LIMITED_JSON", os.path.join(ROOT, "gpurun_out", "f32_limited.json"))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(tolerances.summary(), violations=bad, patches=tolerances.RECORDS), f, indent=1)
    except OSError:
        pass
    if bad and exitstatus == 0:
        print("\nFAILED tests/tolerances.py session bounds: " + "; ".join(bad))
        session.exitstatus = 1
