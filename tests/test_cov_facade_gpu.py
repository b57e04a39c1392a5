"""The facade's PropagateCovariance and InflateCircleTrack (include/altro/altro.hpp) against the C calls, bit for bit, on the
unicycle case of tests/test_cov_gpu.py's parity test (kTurn90, N = 8, batch 3, a different x0 per instance)."""
import os
import subprocess

import numpy as np
import pytest

from test_cov_gpu import _inputs, _x0s

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, ROWS, KAPPA = 8, 3, 5, 1.5


def _bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/cov_facade_driver.cpp: Solve, PropagateCovariance, InflateCircleTrack, printing hexadecimal floats; the C
    calls on the same inputs give the same bits."""
    exe = str(tmp_path / "cov_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "cov_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    x0 = _x0s(B, np.zeros(3))
    Sigma0, W = _inputs(B, 3, N, 21)
    r_ = np.arange(ROWS, dtype=np.float64)
    base = np.stack([5.0 - 0.01 * r_, 5.0 + 0.02 * r_, 0.1 + 0.01 * r_], axis=1)
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), Sigma0.ravel(), W.ravel(), base.ravel()]).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N), str(ROWS), repr(KAPPA)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows[f[0]] = int(f[1]) if f[0] in ("status", "index") else np.array([float.fromhex(v) for v in f[1:]])
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(x0)
    idx = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3)
    assert idx == rows["index"]
    # the driver's per-knot loop of far circles (5 + 1e-3 k, 5, 0.1), as the facade emits it: N + 1 rows, the rows in front of
    # and behind [1, N) repeat its ends
    seed = np.zeros((N + 1, 3))
    seed[:, 0] = 5.0 + 1e-3 * np.clip(np.arange(N + 1), 1, N - 1)
    seed[:, 1], seed[:, 2] = 5.0, 0.1
    s.set_constraint_track(idx, seed)
    s.solve()
    assert rows["status"] == s.get_stats()["status"][0]
    got = s.cov_propagate(N, Sigma0, W)
    for k in ("Sigma", "sx", "su", "rpos"):
        assert _bits(rows[k], got[k].ravel()), k
    assert np.abs(got["Sigma"]).max() > 0
    s.cov_inflate_circles(idx, base, KAPPA, got["rpos"])
    par = s.get_knot_params(idx)
    assert _bits(rows["params"], par.ravel())
    assert (par[:, :, 2] > 0.1).all()
    s.close()
