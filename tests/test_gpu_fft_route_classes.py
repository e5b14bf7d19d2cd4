"""One engine per route class of the FFT engine's default route table (tests/golden/fft_route_table.txt; cases in tests/route_cases.py).

The table is checked against fft_route on the CPU (tests/san/capi_san_driver.cpp); what it cannot show is whether the configure calls
made FROM a route match what the route's launches need -- a kernel whose dynamic-LDS limit was not raised fails at launch. So each
class creates its engine and runs both entries once: the pair entry on frames (1, 0) and (2, 1), the video entry on the three frames.

Bar: kernel_variant as the table's row implies, and every patch of both entries within tolerances.TOL (1e-4 px) of BOTH oracles in the
engine's peak model -- no relaxation, no unpinned escape: test_route_cases_host.py asserts on the CPU that on these inputs the two
oracles are within 2e-5 px of each other and that nothing in the pixels would relax a bar."""
import numpy as np
import pytest
import torch

import route_cases as R
from mrs_optic_flow_amd import FftMethod
from tolerances import TOL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("model,n", list(R.CASES))
def test_class_runs_both_entries_on_its_route(gpu, model, n):
    c = R.case(model, n)
    fm = FftMethod(sample_point_size=n, frame_shape=c.shape, grid=(2, 1), peak_model=model, search_radius=R.SEARCH_RADIUS)
    want = R.variant(R.default_table()[(model, n)])
    assert fm.kernel_variant == want, (model, n, fm.kernel_variant, want)
    frames = torch.from_numpy(c.frames.copy()).to(gpu)  # (the shared case stays read-only)
    pairs = fm.process_batch_device(frames[1:].contiguous(), frames[:-1].contiguous()).cpu().numpy()
    video = fm.process_sequence_device(frames).cpu().numpy()
    for what, got in (("pair entry", pairs), ("video entry", video)):
        assert got.shape == c.want64.shape, (what, got.shape)
        e64, e32 = np.abs(got - c.want64).max(), np.abs(got - c.want32).max()
        print(f"model {model} n {n} {fm.kernel_variant} {what}: max |got - f64 oracle| {e64:.2e} px, |got - f32 oracle| {e32:.2e} px")
        assert np.isfinite(got).all() and e64 <= TOL and e32 <= TOL, (model, n, what, got.tolist(), c.want64.tolist(), c.want32.tolist())
