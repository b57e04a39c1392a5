#!/usr/bin/env python3
"""What the time-varying LQR tracking gains cost (include/altro_lqr.h).

problems.unicycle_turn90 (unicycle, N = 100, control bound and goal constraint, fp64) at batch 4096, solved once; then, host
clock around work that ends in a device synchronise, medians of runs that alternate in one process:
  device   lqr_gains_device with Q, R, Qf, K, P and fail in device memory, nothing installed: k_lqr_linearise + k_lqr_recur +
           k_lqr_install;
  host     the composition it replaces: get_trajectory, update_expansions (which overwrites the handle's expansion records),
           N x get_expansion, and the recursion in numpy, batched over the instances.
The two are checked to agree to 1e-9 of the largest entry first.  Nothing here is asserted as a speed; the figures go into
DESIGN.md as measured.  Prints one JSON line and writes it to --out.

    python scripts/lqr_gains_time.py [--batch 4096] [--reps 10] [--out profiles/lqr_gains_time.json]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

N = 100
Q = np.diag([0.5, 1.25, 2.0])
R = np.array([[0.1, 0.01], [0.01, 1.0]])
QF = 10.0 * Q


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(f, *a):
    t0 = time.perf_counter()
    out = f(*a)
    return (time.perf_counter() - t0) * 1e3, out


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBuffer:
    def __init__(self, hip, nbytes, fill=None):
        self.hip, self.nbytes = hip, nbytes
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes)) == 0
        self.ptr = p.value
        if fill is not None:
            a = np.ascontiguousarray(fill, dtype=np.float64)
            assert hip.hipMemcpy(p, a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), ctypes.c_int(1)) == 0

    def read(self, shape, dtype=np.float64):
        out = np.empty(shape, dtype=dtype)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes), ctypes.c_int(2)) == 0
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def host_composition(s):
    """getters, update_expansions, N x get_expansion, numpy -> K [B][N][m][n], P [B][N + 1][n][n]"""
    B, n, m = s.batch, s.n, s.m
    s.get_trajectory()  # (what a caller reads to know the plan; the expansions are evaluated at it)
    s.update_expansions()
    ex = [s.get_expansion(k) for k in range(N)]
    T = lambda M: np.swapaxes(M, 1, 2)  # noqa: E731
    P = np.empty((B, N + 1, n, n))
    K = np.empty((B, N, m, n))
    P[:, N] = QF
    for k in range(N - 1, -1, -1):
        Ak, Bk = ex[k]["A"], ex[k]["B"]
        PA, PB = P[:, k + 1] @ Ak, P[:, k + 1] @ Bk
        S, G = R + T(Bk) @ PB, T(Bk) @ PA
        K[:, k] = -np.linalg.solve(S, G)
        Pk = Q + T(Ak) @ PA + T(G) @ K[:, k]
        P[:, k] = (Pk + T(Pk)) / 2
    return K, P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lqr_gains_time.json"))
    args = ap.parse_args()
    graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    B = args.batch
    s = P.unicycle_turn90(P.make_hip, batch=B, N=N)
    s.solve()
    hip = hip_runtime()
    dQ, dR, dQf = DeviceBuffer(hip, Q.nbytes, Q), DeviceBuffer(hip, R.nbytes, R), DeviceBuffer(hip, QF.nbytes, QF)
    dK, dP, dfail = DeviceBuffer(hip, 8 * B * N * 6), DeviceBuffer(hip, 8 * B * (N + 1) * 9), DeviceBuffer(hip, 4 * B)

    def device():
        s.lqr_gains_device(dQ.ptr, dR.ptr, dQf.ptr, False, dK.ptr, dP.ptr, dfail.ptr)
    device()
    Kh, Ph = host_composition(s)
    Kd = np.swapaxes(dK.read((B, N, 3, 2)), 2, 3)  # column-major m x n per knot
    Pd = dP.read((B, N + 1, 3, 3))
    assert (dfail.read((B,), np.int32) == -1).all()
    worst = max(float(np.abs(Kd - Kh).max() / np.abs(Kh).max()), float(np.abs(Pd - Ph).max() / np.abs(Ph).max()))
    assert worst < 1e-9, worst
    t_dev, t_host = [], []
    for _ in range(args.reps):
        t_dev.append(timed(device)[0])
        t_host.append(timed(host_composition, s)[0])
    name, _ = s.device_info()
    line = json.dumps(dict(metric="lqr_gains_time", problem="kTurn90 fp64, N = 100", batch=B, reps=args.reps, device=name,
                           device_ms=summary(t_dev), host_composition_ms=summary(t_host), agreement=worst))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for b in (dQ, dR, dQf, dK, dP, dfail):
        b.free()
    s.close()


if __name__ == "__main__":
    main()
