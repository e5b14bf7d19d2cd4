"""Writes tests/golden/ref_cl_bm.npz and tests/golden/ref_cl_fft_peak.npz: inputs, geometry and the outputs of the REFERENCE'S OWN
OpenCL text, executed on the CPU (oracle/cl_host.h; needs oracle/_ref/libref_*.so, i.e. a build() where the reference checkout
exists), for a subset of the cases of tests/ref_cl.py. The files hold data only.

    python tests/golden/make_ref_cl_fixtures.py

tests/test_ref_cl_host.py::test_fixtures_reproduce regenerates both in memory and compares every byte; test_recorded_* hold the
oracle to them on machines without the reference; tests/test_gpu_ref_cl.py holds the kernels to them.

ref_cl_bm.npz       names[k], params[k] = (block, step, radius, scan_block), cur{k} / prev{k} (uint8 frames), dx{k} / dy{k}
                    (int8 [gy, gx]), top_x[k] / top_y[k] (the three most frequent shifts per axis, as the text orders them).
                    The 1 x 1 case records the text's unsorted Y list (the known reference defect).
ref_cl_fft_peak.npz per n in 32 / 64 / 120: cur{n} / prev{n} (uint8 [10, n, n] patch pairs), pair_ref{n} float32 [10, 3, 2]: the
                    text's result on the oracle's f32 surface of pair k placed at patch (0, 0), (6, 6), (2, 5) of a 7 x 7 field (the
                    GPU test runs each pair as a frame of its own, patch (0, 0)); pair_ok{n}: the oracle's second-peak filter.
                    synthetic_names32 / synthetic32 / synthetic_ref32 [m, 3, 2]: a subset of the synthetic 32 x 32 surfaces
                    (ref_cl.recorded_synthetic) and the text's results at the same three origins."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ref_cl as R  # noqa: E402


def bm_arrays():
    cases = R.bm_recorded_cases()
    out = {"names": np.array([c.name for c in cases]),
           "params": np.array([(c.block, c.step, c.radius, c.scan_block) for c in cases], np.int32)}
    tx, ty = [], []
    for k, c in enumerate(cases):
        dx, dy, x3, y3 = R.bm_reference(c)
        out[f"cur{k}"], out[f"prev{k}"], out[f"dx{k}"], out[f"dy{k}"] = c.cur, c.prev, dx, dy
        tx.append(x3)
        ty.append(y3)
    out["top_x"], out["top_y"] = np.array(tx, np.int8), np.array(ty, np.int8)
    return out


def fft_peak_arrays():
    out = {}
    for n in R.PEAK_SIZES:
        pairs = R.patch_pairs(n)
        frame = np.full((R.FIELD * n, R.FIELD * n), 1000.0, np.float32)
        ref = np.zeros((len(pairs), len(R.PEAK_ORIGINS), 2), np.float32)
        ok = np.zeros(len(pairs), np.bool_)
        for k, (cur, prev) in enumerate(pairs):
            surf, diag = R.pair_surface(cur, prev)
            ok[k] = diag["second_value"] < 0.5 * diag["peak_value"]
            for j, (xv, yv) in enumerate(R.PEAK_ORIGINS):
                ref[k, j] = R.peak_reference(surf, xv, yv, frame)
        out[f"cur{n}"] = np.stack([p[0] for p in pairs])
        out[f"prev{n}"] = np.stack([p[1] for p in pairs])
        out[f"pair_ref{n}"], out[f"pair_ok{n}"] = ref, ok
    syn = R.recorded_synthetic(32)
    frame = np.full((R.FIELD * 32, R.FIELD * 32), 1000.0, np.float32)
    out["synthetic_names32"] = np.array([s[0] for s in syn])
    out["synthetic32"] = np.stack([s[1] for s in syn])
    out["synthetic_ref32"] = np.array([[R.peak_reference(s, xv, yv, frame) for xv, yv in R.PEAK_ORIGINS] for _, s in syn], np.float32)
    return out


if __name__ == "__main__":
    assert R.usable(), f"{R.REF_OUT} lacks the reference-text libraries (build where the reference checkout exists)"
    for fname, arrays in (("ref_cl_bm.npz", bm_arrays()), ("ref_cl_fft_peak.npz", fft_peak_arrays())):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **arrays)
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
