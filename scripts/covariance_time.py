#!/usr/bin/env python3
"""What the closed-loop covariance costs (include/altro_covariance.h).

problems.unicycle_turn90 (unicycle, N = 100, control bound and goal constraint, fp64) at batch 4096, solved once; then, host
clock around work that ends in a device synchronise, medians of runs that alternate in one process:
  device   cov_propagate_device(N) with Sigma0, W and all four outputs in device memory: k_cov_linearise + k_cov_recur;
  host     the composition it replaces: get_trajectory, get_gains, update_expansions (which overwrites the handle's expansion
           records), N x get_expansion, and the recursion with Sigma, sx, su and rpos in numpy, batched over the instances.
The two are checked to agree to 1e-9 of the largest entry first.  Nothing here is asserted as a speed; the figures go into
DESIGN.md as measured.  Prints one JSON line and writes it to --out.

    python scripts/covariance_time.py [--batch 4096] [--reps 10] [--out profiles/covariance_time.json]
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
SIGMA0 = np.diag([4e-4, 4e-4, 1e-4])
W = np.diag([1e-5, 1e-5, 1e-6])


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

    def read(self, shape):
        out = np.empty(shape)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes), ctypes.c_int(2)) == 0
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def host_composition(s):
    """getters, update_expansions, N x get_expansion, numpy -> Sigma, sx, su, rpos"""
    B, n = s.batch, s.n
    s.get_trajectory()  # (what a caller reads to know the plan; the expansions are evaluated at it)
    K, _ = s.get_gains()
    s.update_expansions()
    Sigma = np.empty((B, N + 1, n, n))
    Sigma[:, 0] = SIGMA0
    for k in range(N):
        e = s.get_expansion(k)
        F = e["A"] + e["B"] @ K[:, k]
        Sigma[:, k + 1] = F @ Sigma[:, k] @ np.swapaxes(F, 1, 2) + W
    root = lambda v: np.sqrt(np.maximum(v, 0.0))  # noqa: E731
    sx = root(np.diagonal(Sigma, axis1=2, axis2=3))
    su = root(np.einsum("bkia,bkac,bkic->bki", K, Sigma[:, :N], K))
    a, b, c = Sigma[:, :, 0, 0], Sigma[:, :, 1, 0], Sigma[:, :, 1, 1]
    rpos = root((a + c) / 2 + np.sqrt(((a - c) / 2) ** 2 + b ** 2))
    return Sigma, sx, su, rpos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    B = args.batch
    s = P.unicycle_turn90(P.make_hip, batch=B, N=N)
    s.solve()
    hip = hip_runtime()
    shapes = dict(Sigma=(B, N + 1, 3, 3), sx=(B, N + 1, 3), su=(B, N, 2), rpos=(B, N + 1))
    d0, dW = DeviceBuffer(hip, SIGMA0.nbytes, SIGMA0), DeviceBuffer(hip, W.nbytes, W)
    out = {k: DeviceBuffer(hip, 8 * int(np.prod(v))) for k, v in shapes.items()}

    def device():
        s.cov_propagate_device(N, d0.ptr, False, dW.ptr, 0, out["Sigma"].ptr, out["sx"].ptr, out["su"].ptr, out["rpos"].ptr)
    device()
    host = host_composition(s)
    worst = 0.0
    for name, want in zip(("Sigma", "sx", "su", "rpos"), host):
        got = out[name].read(shapes[name])
        worst = max(worst, float(np.abs(got - want).max() / np.abs(want).max()))
    assert worst < 1e-9, worst
    t_dev, t_host = [], []
    for _ in range(args.reps):
        t_dev.append(timed(device)[0])
        t_host.append(timed(host_composition, s)[0])
    name, _ = s.device_info()
    line = json.dumps(dict(metric="covariance_time", problem="kTurn90 fp64, N = 100", batch=B, reps=args.reps, device=name,
                           device_ms=summary(t_dev), host_composition_ms=summary(t_host), agreement=worst))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    for b in list(out.values()) + [d0, dW]:
        b.free()
    s.close()


if __name__ == "__main__":
    main()
