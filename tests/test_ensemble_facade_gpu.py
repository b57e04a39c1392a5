"""The facade's TrackEnsemble, FillNoise and PerturbControlsGaussian (include/altro/altro.hpp) against the C calls, bit for bit,
on kTurn90 (N = 8, batch 3, a different x0 per instance, 70 samples)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B, S, SEED, BASE, TOL = 8, 3, 70, 20261020, 4, 1e-3


def _bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def _psd(rng, shape, scale):
    G = rng.randn(*shape, 3, 3)
    return scale * (G @ np.swapaxes(G, -1, -2))


def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/ens_facade_driver.cpp: Solve, TrackEnsemble, FillNoise, PerturbControlsGaussian, printing hexadecimal floats;
    the C calls on the same inputs give the same bits."""
    exe = str(tmp_path / "ens_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "ens_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rng = np.random.RandomState(21)
    b = np.arange(B, dtype=np.float64)
    x0 = np.stack([0.05 * b, -0.04 * b, 0.03 * b], axis=1)
    Sigma0, W = _psd(rng, (B,), 1e-4), _psd(rng, (B, N), 1e-6)
    lo, hi, sigma = np.array([-1.0, -1.2]), np.array([1.0, 1.2]), np.array([0.05, 0.1])
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), Sigma0.ravel(), W.ravel(), lo, hi, sigma]).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N), str(S), str(SEED), str(BASE), repr(TOL)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        rows[f[0]] = int(f[1]) if f[0] == "status" else np.array([float.fromhex(v) for v in f[1:]])
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(x0)
    s.solve()
    assert rows["status"] == s.get_stats()["status"][0]
    got = s.mpc_ensemble(N, S, seed=SEED, instance_base=BASE, Sigma0=Sigma0, W=W, u_lo=lo, u_hi=hi, viol_tol=TOL,
                         want=("dev_mean", "dev_mom2", "alive", "viol_count", "summary", "stats"))
    for k in ("dev_mean", "dev_mom2", "alive", "viol_count"):
        assert _bits(rows[k], got[k].ravel()), k
    for name, key in (("summary", "summary"), ("stats", "stats")):
        flat = np.stack([got[key][f].astype(np.float64).ravel() for f in got[key].dtype.names], axis=1)
        assert _bits(rows[name], flat.ravel()), name
    assert (got["stats"]["max_dx"] > 0).all() and (got["alive"] == S).all()
    fill = s.noise_fill(N, S, seed=SEED, instance_base=BASE, Sigma0=Sigma0, W=W)
    assert _bits(rows["dx0"], fill["dx0"].ravel()) and _bits(rows["w"], fill["w"].ravel())
    U0 = s.get_trajectory()[1]
    s.multistart_perturb_gaussian(1, SEED, sigma, instance_base=BASE, keep_first=False)
    U1 = s.get_trajectory()[1]
    assert _bits(rows["U"], U1.ravel()) and (U1 != U0).any()
    s.close()
