#!/usr/bin/env python3
"""What event-triggered re-planning saves (include/altro_trigger.h).

kTurn90-sized handles (problems.batch_turn90: unicycle, N = 100, control bound and goal constraint, fp64, a goal per instance) at
batch 1024 and 4096 run 20 closed-loop cycles of shift 5 under a fixed disturbance: a sinusoid of 1e-3 on every state of every
instance, plus ONE pulse of 5e-2 in y on a fraction of the instances (--pulse-fraction), each in a cycle of its own.  Compared,
alternating in one process, medians behind a warm-up round, host clock around calls that end in a device synchronise:
  tracked        mpc_run_tracked: every instance re-solved every cycle (unchanged code: what the library did before);
  tracked_masked the same call on a handle that carries a mask of all ones (include/altro_subset.h): the same solves started
                 the way a masked solve starts.  tracked_masked - tracked is what the masked start alone changes, and
                 max_age 1 - tracked_masked what the rule, the compaction and the log kernel cost on top;
  max_age A      mpc_run_triggered with dx_tol 2e-2 (only a pulse exceeds it) and max_age A in {1, 2, 4, 19}.  max_age 1
                 re-solves everyone every cycle through the masked path: against `tracked` it shows what the rule, the masks
                 and the log kernel cost; 19 re-plans by deviation alone (a plan of N = 100 can be followed for 19 cycles).
Per run: ms per cycle, solves per cycle, the summed tracked cost and the largest tracked violation of what the run applied.
Also: the run-to-run spread (max - min) of `tracked` itself, and the time of one trigger evaluation plus mask compaction alone
(mpc_trigger_device + set_solve_mask_device on device arrays).  The figure to read: max_age 1 against tracked should differ by no
more than that spread plus one evaluation time, all per cycle; `max_age_1_within_spread` says whether it did.
Prints one JSON line and writes it to --out.

    python scripts/triggered_time.py [--batches 1024,4096] [--reps 5] [--pulse-fraction 0.1] [--out profiles/triggered_run.json]
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

N, SHIFT, CYCLES = 100, 5, 20
AGES = (1, 2, 4, 19)
SINE, PULSE, DX_TOL = 1e-3, 5e-2, 2e-2
LO, HI = np.array([-1.5, -1.5]), np.array([1.5, 1.5])


def summary(ms):
    return dict(median=float(np.median(ms)), min=float(np.min(ms)), max=float(np.max(ms)))


def timed(f, *a, **kw):
    t0 = time.perf_counter()
    out = f(*a, **kw)
    return (time.perf_counter() - t0) * 1e3, out


def disturbance(B, n, fraction):
    """w [CYCLES][B][SHIFT][n]: SINE sin(1 + 3 c + 5 b + 7 i + 11 k) everywhere; every round(1 / fraction)-th instance gets
    PULSE in y at knot 0 of cycle 1 + (its rank among the pulsed) % (CYCLES - 1)"""
    c, b, k, i = np.meshgrid(np.arange(CYCLES), np.arange(B), np.arange(SHIFT), np.arange(n), indexing="ij")
    w = SINE * np.sin(1.0 + 3.0 * c + 5.0 * b + 7.0 * i + 11.0 * k)
    pulsed = np.arange(0, B, max(int(round(1.0 / fraction)), 1)) if fraction > 0 else np.arange(0)
    for rank, inst in enumerate(pulsed):
        w[1 + rank % (CYCLES - 1), inst, 0, 1] += PULSE
    return np.ascontiguousarray(w), int(pulsed.size)


class DeviceArray:
    """device memory holding the bytes of a numpy array (the HIP runtime the solver library has loaded, through ctypes)"""

    def __init__(self, data):
        data = np.ascontiguousarray(data)
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.hip = ctypes.CDLL(path)
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(data.nbytes, 1))) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), data.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(data.nbytes), ctypes.c_int(1)) == 0

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def measure(A, P, batch, reps, fraction):
    s = P.batch_turn90(P.make_hip, batch, N=N)
    w, pulsed = disturbance(batch, s.n, fraction)
    x0 = np.zeros((batch, s.n))
    rules = {age: dict(max_age=age, dx_tol=DX_TOL, viol_tol=-1.0, on_unsolved=0, lookahead=0, ahead_tol=0.0) for age in AGES}

    def run(name):
        s.reset_trajectory()  # every run starts from the same guess and the same state
        s.set_initial_state(x0)
        if name == "tracked":
            return timed(s.mpc_run_tracked, CYCLES, SHIFT, w=w, u_lo=LO, u_hi=HI)
        if name == "tracked_masked":
            s.set_solve_mask(np.ones(batch, bool))
            out = timed(s.mpc_run_tracked, CYCLES, SHIFT, w=w, u_lo=LO, u_hi=HI)
            s.set_solve_mask(None)
            return out
        return timed(s.mpc_run_triggered, CYCLES, SHIFT, rules[name], w=w, u_lo=LO, u_hi=HI)
    names = ("tracked", "tracked_masked") + AGES
    t = {name: [] for name in names}
    last = {}
    for rep in range(1 + reps):  # the first round warms up: code objects, staging buffers, the run's blocks
        for name in names:
            ms, out = run(name)
            if rep > 0:
                t[name].append(ms / CYCLES)
            last[name] = out
    # one evaluation of the rule plus the compaction of its mask, on device arrays: the statistics of a real cycle
    d_stats, d_age = DeviceArray(last[1]["track"][:, CYCLES - 1].copy()), DeviceArray((np.arange(batch) % 4).astype(np.int32))
    d_mask, d_why = DeviceArray(np.zeros(batch, np.uint8)), DeviceArray(np.zeros(batch, np.int32))
    t_eval = []
    for _ in range(3 + 10):
        t0 = time.perf_counter()
        s.mpc_trigger_device(rules[2], d_stats.ptr, d_age.ptr, 0, 0, d_mask.ptr, d_why.ptr)
        s.set_solve_mask_device(d_mask.ptr)
        t_eval.append((time.perf_counter() - t0) * 1e3)
    s.set_solve_mask(None)
    for d in (d_stats, d_age, d_mask, d_why):
        d.free()
    rows = {}
    for name in names:
        out = last[name]
        solved = out["reason"] != 0 if name in AGES else out["iterations"] > 0
        rows[str(name)] = dict(ms_per_cycle=summary(t[name]), solves_per_cycle=float(solved.sum()) / CYCLES,
                               tracked_cost_sum=float(out["track"]["cost"].sum()), tracked_violation_max=float(out["track"]["violation"].max()),
                               limits_hit=int((out["track"]["status"] != A.UNSOLVED).sum()))
    spread = float(np.max(t["tracked"]) - np.min(t["tracked"]))
    evaluation = float(np.median(t_eval[3:]))
    diff = float(np.median(t[1]) - np.median(t["tracked"]))
    same = all(np.array_equal(last[name][k], last["tracked"][k]) for name in (1, "tracked_masked") for k in ("X_cl", "U_cl", "iterations", "status"))
    s.close()
    return dict(batch=batch, reps=reps, pulsed_instances=pulsed, runs=rows, tracked_spread_ms_per_cycle=spread,
                trigger_eval_and_compaction_ms=summary(t_eval[3:]), max_age_1_minus_tracked_ms_per_cycle=diff,
                tracked_masked_minus_tracked_ms_per_cycle=float(np.median(t["tracked_masked"]) - np.median(t["tracked"])),
                max_age_1_minus_tracked_masked_ms_per_cycle=float(np.median(t[1]) - np.median(t["tracked_masked"])),
                max_age_1_within_spread=bool(abs(diff) <= spread + evaluation), max_age_1_same_bits_as_tracked=bool(same))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1024,4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pulse-fraction", type=float, default=0.1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triggered_run.json"))
    args = ap.parse_args()
    A = graft.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    rows = [measure(A, P, int(b), args.reps, args.pulse_fraction) for b in args.batches.split(",")]
    probe = P.unicycle_turn90(P.make_hip, batch=1, N=N)
    probe.rollout()
    name, _ = probe.device_info()
    line = json.dumps(dict(metric="triggered_run", problem="kTurn90 fp64, N = 100, a goal per instance", shift=SHIFT, cycles=CYCLES,
                           sine=SINE, pulse=PULSE, dx_tol=DX_TOL, pulse_fraction=args.pulse_fraction, device=name, rows=rows))
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
