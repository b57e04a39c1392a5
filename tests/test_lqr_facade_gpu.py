"""The facade's SetLqrGainPolicy, ClearLqrGainPolicy and ComputeLqrGains (include/altro/altro.hpp) against the C calls, bit for
bit, on the unicycle (kTurn90, N = 24, batch 5, a different x0 per instance)."""
import os
import subprocess

import numpy as np
import pytest

import _lqr_common as LC
from test_cov_gpu import _x0s

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = 24, 5


def _bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/lqr_facade_driver.cpp: SetLqrGainPolicy, Solve, altro_get_gains, ClearLqrGainPolicy, ComputeLqrGains, printing
    hexadecimal floats; the C calls on the same inputs give the same bits, and the policy's gains are the direct call's."""
    exe = str(tmp_path / "lqr_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "lqr_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    x0 = _x0s(B, np.zeros(3))
    Q, R, Qf = LC.parity_weights(3, 2)
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), Q.ravel(), R.ravel(), Qf.ravel()]).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows[f[0]] = int(f[1]) if f[0] == "status" else np.array([float.fromhex(v) for v in f[1:]])
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(x0)
    s.solve()
    assert rows["status"] == s.get_stats()["status"][0]
    got = s.lqr_gains(Q, R, Qf)
    Kc = np.swapaxes(got["K"], 2, 3)  # [B][N][m n], column-major m x n: the C layout the driver prints
    assert _bits(rows["K"], Kc.ravel()) and _bits(rows["P"], got["P"].ravel())
    assert (rows["fail"] == got["fail"]).all() and (got["fail"] == -1).all()
    assert _bits(rows["policy_K"], Kc.ravel()) and (rows["policy_d"] == 0).all()
    assert np.abs(got["K"]).max() > 0
    s.close()
