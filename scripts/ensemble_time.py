#!/usr/bin/env python3
"""Times the Monte-Carlo ensemble (include/altro_ensemble.h) on kTurn90, fp64, N = 100, for B in {64, 4096} and S in {64, 1024},
against the two ways a caller had before it, and writes profiles/ensemble_time.json:

  ensemble     altro_mpc_ensemble_device: noise drawn in the kernel, per-knot moments and counts reduced on the device
  host_way     numpy noise on the host, upload, altro_mpc_track_device with statistics only, download, host reduction of the
               statistics (no per-knot moments: the track has none to give without its logs).  Skipped ("not measured") where
               the noise alone exceeds --host-limit bytes.
  chain_only   altro_mpc_track_device with dx0 and w already resident (filled by altro_noise_fill_device): the chain alone

Host clocks around calls that end in a synchronise; the variants alternate within every repetition and the medians are kept.
No time here is a pass bar.  Needs a GPU: there is no CPU fallback."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class Dev:
    def __init__(self, hip, nbytes):
        self.hip, self.nbytes = hip, nbytes
        p = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(nbytes, 1))) != 0:
            raise MemoryError(f"hipMalloc of {nbytes} bytes")
        self.ptr = p.value

    def put(self, a):
        a = np.ascontiguousarray(a)
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), a.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(a.nbytes), ctypes.c_int(1)) == 0

    def get(self, like):
        assert self.hip.hipMemcpy(like.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(like.nbytes), ctypes.c_int(2)) == 0
        return like

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-limit", type=float, default=2e9, help="largest host noise array (bytes) the host way is timed with")
    ap.add_argument("--batches", type=int, nargs="*", default=[64, 4096])
    ap.add_argument("--samples", type=int, nargs="*", default=[64, 1024])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_time.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = __import__("altro_cpp_amd.problems", fromlist=["x"])
    N, n = 100, 3
    Sigma0, W = np.diag([4e-4, 4e-4, 1e-4]), np.diag([1e-5, 1e-5, 1e-6])
    L0, Lw = np.linalg.cholesky(Sigma0), np.linalg.cholesky(W)
    rows = []
    for B in args.batches:
        s = P.batch_turn90(lambda n_, m_, N_, b_, d_: A.BatchSolver(n_, m_, N_, b_, d_), batch=B, N=N)
        s.solve()
        hip = hip_runtime()
        dS0, dW = Dev(hip, 72), Dev(hip, 72)
        dS0.put(Sigma0), dW.put(W)
        for S in args.samples:
            K1 = N + 1
            mean, mom2 = Dev(hip, B * K1 * n * 8), Dev(hip, B * K1 * n * n * 8)
            alive, viol, summ = Dev(hip, B * K1 * 4), Dev(hip, B * K1 * 4), Dev(hip, B * A.ENSEMBLE_STATS_DTYPE.itemsize)
            dx0, w = Dev(hip, B * S * n * 8), Dev(hip, B * S * N * n * 8)
            stats = Dev(hip, B * S * A.TRACK_STATS_DTYPE.itemsize)
            host_stats = np.zeros((B, S), dtype=A.TRACK_STATS_DTYPE)
            host_ok = w.nbytes <= args.host_limit
            rng = np.random.RandomState(1)

            def ensemble(seed):
                s.mpc_ensemble_device(N, S, seed, 0, dS0.ptr, False, dW.ptr, 0, 0, 0, 1e-3, mean.ptr, mom2.ptr, alive.ptr, viol.ptr, summ.ptr, 0)

            def host_way(seed):
                a = rng.standard_normal((B, S, n)) @ L0.T
                b = rng.standard_normal((B, S, N, n)) @ Lw.T
                dx0.put(a), w.put(b)
                s.mpc_track_device(N, S, dx0.ptr, w.ptr, 0, 0, 0, 0, stats.ptr)
                st = stats.get(host_stats)
                done = st["status"] == A.UNSOLVED
                return (np.where(done, st["cost"], 0.0).sum(axis=1) / np.maximum(done.sum(axis=1), 1), st["violation"].max(axis=1),
                        (st["violation"] > 1e-3).sum(axis=1))

            def chain_only(seed):
                s.mpc_track_device(N, S, dx0.ptr, w.ptr, 0, 0, 0, 0, stats.ptr)

            variants = [("ensemble", ensemble), ("chain_only", chain_only)] + ([("host_way", host_way)] if host_ok else [])
            s.noise_fill_device(N, S, 1, 0, dS0.ptr, False, dW.ptr, 0, dx0.ptr, w.ptr)  # (what chain_only runs on)
            for _, fn in variants:  # warm-up of every variant at this shape
                fn(0)
            times = {name: [] for name, _ in variants}
            for r in range(args.reps):
                for name, fn in variants:
                    t0 = time.perf_counter()
                    fn(r + 1)
                    times[name].append(time.perf_counter() - t0)
            row = dict(B=B, S=S, N=N, reps=args.reps, noise_bytes=w.nbytes)
            for name in ("ensemble", "host_way", "chain_only"):
                row[name + "_ms"] = 1e3 * float(np.median(times[name])) if name in times else None
                row[name + "_all_ms"] = [1e3 * t for t in times[name]] if name in times else "not measured"
            print(json.dumps(row), flush=True)
            rows.append(row)
            for d in (mean, mom2, alive, viol, summ, dx0, w, stats):
                d.free()
        dS0.free(), dW.free()
        name, cus = s.device_info()
        s.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=name, compute_units=cus, model="kTurn90 fp64", rows=rows), f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
