"""CPU tests of the estimator's correlation quality and response gate (include/mof.h, mof_sr_*_q, mof_sr_set_min_response): the new
entries exist and refuse a null engine, and the reference test_gpu_sr_quality.py is held to -- tests/sr_quality_cases.py, a state
machine around the unchanged oracle's log-polar remap and phase correlation -- is itself proven: with the response gate off it is the
oracle's estimator to the bit, its gate inputs separate from the threshold with room on both sides, and the distance of the two
oracles the GPU bar is a multiple of is not zero."""
import numpy as np
import pytest

import oracle_lib as O
import sr_quality_cases as S
from mrs_optic_flow_amd import _capi

NEW_SYMBOLS = ("mof_sr_process_q", "mof_sr_process_batch_device_q", "mof_sr_process_sequence_device_q", "mof_sr_process_sequence_host_q",
               "mof_sr_set_min_response", "mof_sr_min_response")


def test_library_exports_the_estimator_quality_entries():
    lib = _capi.load()  # (resolves every symbol of its table, these six among them)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f"{name} is not exported by {_capi.LIB_PATH}"


def test_q_entries_and_the_setter_refuse_a_null_engine():
    lib = _capi.load()
    nil = None
    assert lib.mof_sr_process_q(nil, nil, 0, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_sr_process_batch_device_q(nil, nil, 0, nil, 0, 0, 1, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_sr_process_sequence_device_q(nil, nil, 0, 0, 1, nil, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_sr_process_sequence_host_q(nil, nil, 0, 0, 1, nil, nil, nil) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_sr_set_min_response(nil, 0.5) == _capi.MOF_ERR_NOT_INIT
    assert lib.mof_sr_min_response(nil) == 0.0


@pytest.mark.parametrize("case", ["views", "reference-gate"])
def test_machine_with_the_gate_off_is_the_oracle_estimator(case):
    """(scale, rot, pt) of every frame, exactly: on the five views (nothing gated) and on a noise video whose frame 6 fails the reference's
    rule, so that frame 7 has an older partner"""
    res, M = 100, 22.0
    frames = S.views(res) if case == "views" else S.reference_gate_video()
    got = S.run_video(frames, res, M)
    ref = O.ScaleRotationEstimator(res, M, 64)
    for k, f in enumerate(frames):
        s, r = ref.processImage(f)
        assert (got.out[k, 0], got.out[k, 1]) == (s, r), (case, k)
        assert (got.out[k, 2], got.out[k, 3]) == ref.pt, (case, k)
    assert np.isnan(got.quality[0]).all() and np.isfinite(got.quality[1:]).all()
    assert got.gated.tolist() == ([False] * len(frames) if case == "views" else [k == 6 for k in range(len(frames))])
    if case == "reference-gate":  # (the gated frame reports the quality of the correlation that gated it; what follows is the older pair's)
        lp5, lp7 = O.logpolar(frames[5], M, S.INTER_LANCZOS4), O.logpolar(frames[7], M, S.INTER_LANCZOS4)
        assert np.array_equal(got.quality[7], S.correlate(lp7, lp5)[1])


@pytest.mark.parametrize("res,M", S.GATE_CASES)
def test_gate_inputs_separate_from_the_threshold(res, M):
    """Every response a gate test compares with MIN_RESPONSE lies at least 1.5 x away from it, on the f64 and on the f32 oracle: no
    precision can flip a decision. If not, the input is wrong, not the bar."""
    refs = S.gate_refs(res, M)
    # which frames / pairs hold the noise frame
    want = dict(video=[k == S.NOISE_AT for k in range(6)], consecutive=[k in (S.NOISE_AT, S.NOISE_AT + 1) for k in range(6)],
                pairs=[k in (S.NOISE_AT - 1, S.NOISE_AT) for k in range(5)])
    for name, noisy in want.items():
        ref = refs[name]
        assert ref.gated.tolist() == noisy, (name, ref.gated.tolist())
        for q in (ref.quality, ref.quality32):
            ran = ~np.isnan(q[:, 0])
            resp, bad = q[ran, 0], np.array(noisy)[ran]
            print(f"{ref.name}: matched >= {resp[~bad].min():.3f}, noise <= {resp[bad].max():.3f}, threshold {S.MIN_RESPONSE}")
            assert resp[~bad].min() >= 1.5 * S.MIN_RESPONSE and resp[bad].max() <= S.MIN_RESPONSE / 1.5
        assert (np.abs(ref.out[ref.gated, 2]) <= res // 2).all()  # the reference's rule is blind to them: pt.x lies inside its gate
    # the gate off: frame 3 becomes the previous image and nothing is gated
    assert not refs["off"].gated.any()
    assert np.array_equal(refs["off"].out[:S.NOISE_AT + 1, 2:], refs["video"].out[:S.NOISE_AT + 1, 2:])
    # frame 4 of the resolved video is the (v3, v2) pair
    v = S.views(res)
    lp = [O.logpolar(v[k], M, S.INTER_LANCZOS4) for k in (2, 3)]
    assert np.array_equal(refs["video"].quality[S.NOISE_AT + 1], S.correlate(lp[1], lp[0])[1])


def test_every_batch_has_a_distance():
    """d > 0: the two oracles differ on every batch, so no GPU bar is zero"""
    batches = [S.route_video(res, M) for res, M in S.ROUTES] + [S.route_pairs(res, M) for res, M in S.ROUTES]
    batches += [S.route_video(100, 22.0, 1), S.route_pairs(100, 22.0, 1)]
    for res, M in S.GATE_CASES:
        batches += list(S.gate_refs(res, M).values())
    for b in batches:
        print(f"{b.name}: d = {b.d:.2e}, bar {b.bar:.2e}")
        assert b.d > 0.0, b.name
