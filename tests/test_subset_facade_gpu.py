"""The solve mask and sequential team rounds through the C++ facade (include/altro/altro.hpp): the driver
tests/cpp/subset_facade_driver.cpp prints hexadecimal floats; the C calls on the same inputs give the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _subset_common as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = SC.N


def _bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and (a.view(np.uint64) == b.view(np.uint64)).all()


def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    T, Ag, sweeps = 2, 3, 1
    B = T * Ag
    exe = str(tmp_path / "subset_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "subset_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    x0, xf = P.team_ring_states(T, Ag)
    rad = np.full(Ag, P.TEAM_RING_RADIUS)
    mask = np.array([1, 0, 1, 1, 0, 0], dtype=bool)
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), xf.ravel(), rad, mask.astype(np.float64)]).tofile(path)
    r = subprocess.run([exe, path, str(T), str(Ag), str(N), str(sweeps)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    traj = {tag: (np.full((B, N + 1, 3), np.nan), np.full((B, N, 2), np.nan)) for tag in ("masked", "sequential")}
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] in traj:
            traj[f[0]][0 if f[1] == "x" else 1][int(f[2]), int(f[3])] = [float.fromhex(v) for v in f[4:]]
        elif f[0] in ("nomask", "mask", "after", "cleared"):
            rows[f[0]] = (int(f[1]), np.array([int(v) for v in f[2:]], dtype=bool))
        elif f[0] in ("status", "index"):
            rows[f[0]] = int(f[1])
    # the same through the C calls (the driver's placeholder circles as the facade emits them: see tests/test_team_gpu.py)
    s = P.unicycle_turn90(hip_make, batch=B, N=N, xf=xf, u0=np.array([0.1, 0.0]))
    s.set_initial_state(x0)
    idx = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3 * (Ag - 1))
    assert idx == rows["index"]
    seed = np.zeros((N + 1, Ag - 1, 3))
    seed[:, :, 0] = (1e-3 * np.clip(np.arange(N + 1), 1, N - 1))[:, None]
    s.set_constraint_track(idx, seed.reshape(N + 1, -1))
    s.solve()
    assert rows["nomask"][0] == B and rows["nomask"][1].all()
    s.team_fill_tracks(Ag, idx, rad)
    s.set_solve_mask(mask)
    assert rows["mask"][0] == int(mask.sum()) and (rows["mask"][1] == mask).all()
    s.solve()
    Xs, Us = s.get_trajectory()
    assert _bits(traj["masked"][0], Xs) and _bits(traj["masked"][1], Us)
    s.team_solve_sequential(Ag, idx, rad, sweeps)
    Xs, Us = s.get_trajectory()
    assert _bits(traj["sequential"][0], Xs) and _bits(traj["sequential"][1], Us)
    assert rows["after"][0] == int(mask.sum()) and (rows["after"][1] == mask).all()
    assert rows["cleared"][0] == B and rows["cleared"][1].all()
    assert rows["status"] == s.get_stats()["status"][0]
    s.close()
