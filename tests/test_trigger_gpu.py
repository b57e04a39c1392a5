"""Event-triggered re-planning on the device (include/altro_trigger.h): the device rule is the numpy rule of
tests/_trigger_common.py; altro_mpc_run_triggered is the caller's own loop over altro_set_solve_mask, altro_solve_al,
altro_mpc_track, altro_mpc_advance and altro_mpc_trigger, bit for bit; max_age = 1 is altro_mpc_run_tracked; an instance that
is not re-planned is untouched by the cycle's solve; the lookahead; the refusals; the facade.  Every problem has N = 24."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _subset_common as SC
import _trigger_common as TG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = TG.N
DX_TOL = 1e-3
LO, HI = np.array([-1.5, -1.5]), np.array([1.5, 1.5])  # problems.unicycle_turn90's control bound
BOUNDS = {"turn90_f64": (LO, HI), "three_obstacles_f32": (np.array([0.0, -3.0]), np.array([3.0, 3.0]))}  # each problem's own


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceArray:
    """device memory holding the bytes of a numpy array (hipMalloc / hipMemcpy through ctypes)"""

    def __init__(self, data):
        self.like = np.ascontiguousarray(data)
        self.hip = _hip_runtime()
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(self.like.nbytes, 1))) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), self.like.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(self.like.nbytes),
                                  ctypes.c_int(1)) == 0  # host to device

    def get(self):
        out = np.empty_like(self.like)
        assert self.hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr), ctypes.c_size_t(out.nbytes),
                                  ctypes.c_int(2)) == 0  # device to host
        return out

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def _w_of(B, steps, n, scale=1e-2):
    """w[b][0][k][i] = scale sin(2 + 5 b + 7 i + 11 k): tests/test_mpc_track_gpu.py's w_of with one sample"""
    b, k, i = np.meshgrid(np.arange(B), np.arange(steps), np.arange(n), indexing="ij")
    return (scale * np.sin(2.0 + 5.0 * b + 7.0 * i + 11.0 * k))[:, None]


def _build(A, P, make, case, B):
    if case == "turn90_f64":
        return P.batch_turn90(make, B, N=N)
    if case == "three_obstacles_f32":
        return P.batch_three_obstacles(make, B, N=N, dtype=A.F32)
    raise KeyError(case)


def _status_of(e):
    return int(str(e.value).split("failed (")[1].split(")")[0])


# ---- 1. the device rule is the numpy rule ---------------------------------------------------------------------------------
def test_device_rule_is_the_numpy_rule(A, P, hip_make):
    """B = 70: more than a wavefront, not a multiple of 64.  The statistics of a real altro_mpc_track(shift = 2) under
    disturbances, ages b % 4; the host and the device form, tracked = NULL, age = NULL, and the device mask straight into
    altro_set_solve_mask_device.  The call changes nothing on the handle."""
    B = 70
    s = _build(A, P, hip_make, "turn90_f64", B)
    s.solve()
    stats = s.mpc_track(2, 1, w=_w_of(B, 2, s.n))["stats"][:, 0]
    age = (np.arange(B) % 4).astype(np.int32)
    status = s.get_stats()["status"]
    # the deviations of this disturbance lie around 1e-2: a tolerance in their middle splits the batch
    rule = TG.rule_dict(max_age=3, dx_tol=float(np.sort(stats["max_dx"])[B // 2]), viol_tol=1e-4, on_unsolved=1)
    before = SC.snapshot(s)
    for tracked, ages in ((stats, age), (None, age), (stats, None), (None, None)):
        want = TG.reason(rule, B, tracked, ages, status)
        mask, why = s.mpc_trigger(rule, tracked=tracked, age=ages)
        assert why.dtype == np.int32 and TG.same_bits(why, want), (tracked is None, ages is None)
        assert np.array_equal(mask, want != 0)
        # the device form
        d_mask, d_why = DeviceArray(np.full(B, 7, dtype=np.uint8)), DeviceArray(np.full(B, -1, dtype=np.int32))
        d_t = DeviceArray(tracked) if tracked is not None else None
        d_a = DeviceArray(ages) if ages is not None else None
        s.mpc_trigger_device(rule, d_t.ptr if d_t else 0, d_a.ptr if d_a else 0, 0, 0, d_mask.ptr, d_why.ptr)
        assert TG.same_bits(d_why.get(), want) and TG.same_bits(d_mask.get(), (want != 0).astype(np.uint8))
        if tracked is not None and ages is not None:
            assert len(set(want.tolist())) >= 4 and 0 in want and (want != 0).any(), set(want.tolist())
            s.set_solve_mask_device(d_mask.ptr)
            assert np.array_equal(s.get_solve_mask(), want != 0)
            s.set_solve_mask(None)
        for d in (d_mask, d_why, d_t, d_a):
            if d:
                d.free()
    # only one of the outputs
    d_mask = DeviceArray(np.zeros(B, dtype=np.uint8))
    s.mpc_trigger_device(rule, mask_ptr=d_mask.ptr)
    assert TG.same_bits(d_mask.get(), (TG.reason(rule, B, None, None, status) != 0).astype(np.uint8))
    d_mask.free()
    assert not SC.differing(SC.snapshot(s), before, np.ones(B, bool))
    s.close()


# ---- 2. the run is the caller's loop, bit for bit; 4. a skipped instance is untouched -----------------------------------------
def _compare_runs(got, ref, label):
    for key in ("X_cl", "U_cl", "iterations", "status", "reason"):
        assert TG.same_bits(got[key], ref[key]), (label, key)
    for field in ref["track"].dtype.names:
        assert TG.same_bits(np.ascontiguousarray(got["track"][field]), np.ascontiguousarray(ref["track"][field])), (label, field)


RUN_CASES = [("turn90_f64", 5, 7), ("three_obstacles_f32", 70, 7), ("turn90_f64", 2112, 4)]


@pytest.mark.parametrize("case,B,cycles", RUN_CASES, ids=[f"{c}_B{B}" for c, B, _ in RUN_CASES])
def test_run_is_the_composed_loop(A, P, hip_make, case, B, cycles):
    """shift 2, max_age = 3, dx_tol = 1e-3; zero disturbance for even instances, for an odd instance b a pulse of 10 dx_tol in
    y at knot 0 of cycle 1 + b % 3.  An undisturbed instance tracks its plan to rounding and triggers by AGE only; a pulse
    adds its full size to the deviation at the next knot and triggers DEVIATION in the next cycle.  What the scenario is meant
    to exercise is asserted on the composed loop alone, before the run is compared.  B = 2112 lies past the 2048 where the
    batch is cut into four chain slices.  It runs four cycles, one more than its three need: behind the full first mask,
    one empty and two partial masks, and AGE with max_age = 3, take cycles 1 to 3 (its first three cycles are the
    three-cycle run).  Every partial mask there must reach every slice.
    In the first configuration the composed loop also takes a snapshot before and after every cycle's solve: an instance with
    reason 0 has identical bits in both."""
    shift = 2
    rule = TG.rule_dict(max_age=3, dx_tol=DX_TOL)
    ref_h, run_h = _build(A, P, hip_make, case, B), _build(A, P, hip_make, case, B)
    w = TG.pulses(cycles, B, shift, ref_h.n, 10 * DX_TOL)
    lo, hi = BOUNDS[case]
    ref = TG.composed_loop(ref_h, cycles, shift, rule, w, lo, hi, snapshot=SC.snapshot if B == 5 else None)
    counts = [int(m.sum()) for m in ref["masks"]]
    print(f"{case} B{B}: solved per cycle {counts}; reasons {sorted(set(ref['reason'].ravel().tolist()))}")
    assert counts[0] == B and (ref["reason"][:, 0] == TG.FIRST).all()
    assert any(c == 0 for c in counts), counts
    partial = [c for c in counts if 0 < c < B]
    assert len(partial) >= 2, counts
    seen = set(ref["reason"].ravel().tolist())
    assert 0 in seen and TG.AGE in seen and any(r & TG.DEVIATION for r in seen), seen
    if B > 2048:
        for part in (m for m in ref["masks"] if 0 < m.sum() < B):
            assert all(part[a:b].any() and not part[a:b].all() for a, b in SC.chain_slices(B))
    assert (ref["iterations"][ref["reason"] == 0] == 0).all() and (ref["iterations"][ref["reason"] != 0] > 0).all()
    # an undisturbed instance stays within dx_tol of its plan and so triggers by AGE only; a pulse adds its full size to whatever
    # deviation there was (the triangle inequality: at least 9 dx_tol are left)
    even = np.arange(B) % 2 == 0
    print("largest deviation of an undisturbed instance:", ref["track"]["max_dx"][even].max())
    assert ref["track"]["max_dx"][even].max() <= DX_TOL and not (ref["reason"][even] & ~(TG.FIRST | TG.AGE)).any()
    assert ref["track"]["max_dx"][~even].max() >= 9 * DX_TOL
    if B == 5:  # 4. a skipped instance is untouched
        skipped = 0
        for c, (before, after) in enumerate(ref["around"]):
            rows = ref["reason"][:, c] == 0
            skipped += int(rows.sum())
            assert not SC.differing(after, before, rows), (c, SC.differing(after, before, rows))
            if (~rows).any():
                assert SC.differing(after, before, ~rows), c
        assert skipped > 0
    got = run_h.mpc_run_triggered(cycles, shift, rule, w=w, u_lo=lo, u_hi=hi)
    _compare_runs(got, ref, f"{case} B{B}")
    a, b = SC.snapshot(run_h), SC.snapshot(ref_h)
    assert not SC.differing(a, b, np.ones(B, bool)), SC.differing(a, b, np.ones(B, bool))
    assert run_h.get_solve_mask().all() and ref_h.get_solve_mask().all()  # the run leaves the handle without a mask
    assert run_h.get_timing()["instance_iterations"] == ref_h.get_timing()["instance_iterations"]
    ref_h.close()
    run_h.close()


# ---- 3. max_age = 1 is altro_mpc_run_tracked ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,B", [("turn90_f64", 5), ("three_obstacles_f32", 70)])
def test_max_age_one_is_run_tracked(A, P, hip_make, case, B):
    cycles, shift = 4, 2
    lo, hi = BOUNDS[case]
    ref_h, run_h = _build(A, P, hip_make, case, B), _build(A, P, hip_make, case, B)
    w = TG.pulses(cycles, B, shift, ref_h.n, 10 * DX_TOL)
    ref = ref_h.mpc_run_tracked(cycles, shift, w=w, u_lo=lo, u_hi=hi)
    got = run_h.mpc_run_triggered(cycles, shift, TG.rule_dict(max_age=1, dx_tol=DX_TOL), w=w, u_lo=lo, u_hi=hi)
    for key in ("X_cl", "U_cl", "iterations", "status"):
        assert TG.same_bits(got[key], ref[key]), key
    for field in ref["track"].dtype.names:
        assert TG.same_bits(np.ascontiguousarray(got["track"][field]), np.ascontiguousarray(ref["track"][field])), field
    assert (got["reason"][:, 0] == TG.FIRST).all() and ((got["reason"][:, 1:] & TG.AGE) != 0).all()
    assert (got["iterations"] > 0).all()
    assert not SC.differing(SC.snapshot(run_h), SC.snapshot(ref_h), np.ones(B, bool))
    ref_h.close()
    run_h.close()


# ---- 5. the lookahead ------------------------------------------------------------------------------------------------------
_PLAN = {}


def _turn90_beside_a_circle(P, make, B):
    """kTurn90 with a circle of radius 0.3 whose centre lies 0.5 above knot 3 of the unconstrained plan: the plan passes
    underneath, 0.2 clear at knot 3 and never nearer than 0.1, so the circle is not active; a plant that finds itself 0.3
    higher in y around those knots is inside it."""
    if "X" not in _PLAN:
        h = P.unicycle_turn90(make, batch=1, N=N)
        h.solve()
        _PLAN["X"] = h.get_trajectory()[0][0]
        h.close()
    X = _PLAN["X"]
    centre = np.array([X[3, 0], X[3, 1] + 0.5])
    gap = np.hypot(X[:, 0] - centre[0], X[:, 1] - centre[1]) - 0.3
    assert gap.min() >= 0.1 and gap[3:6].max() <= 0.2 + 1e-12, gap[:8]
    s = P.unicycle_turn90(make, batch=B, N=N)
    s.add_circle_constraint(1, N, np.array([[centre[0], centre[1], 0.3]]))
    return s


def test_lookahead(A, P, hip_make):
    """dx_tol and viol_tol off, lookahead = 6, ahead_tol = the problem's constraint tolerance.  After a solve nobody has AHEAD;
    with half the instances moved by 0.3 in y exactly those have it.  The statistics behind the bit are those of
    altro_mpc_track(6, 1) from the same handle state, pushed through the numpy rule."""
    B, L = 70, 6
    s = _turn90_beside_a_circle(P, hip_make, B)
    tol = s.get_options().constraint_tolerance
    rule = TG.rule_dict(max_age=4, lookahead=L, ahead_tol=tol)
    with pytest.raises(A.AltroError) as e:  # (no gains yet)
        s.mpc_trigger(rule)
    assert _status_of(e) == A.NOT_READY and "gains" in str(e.value)
    s.solve()
    assert (s.get_stats()["status"] == A.SOLVED).all()
    before = SC.snapshot(s)
    ahead = s.mpc_track(L, 1, log=False)["stats"][:, 0]
    mask, why = s.mpc_trigger(rule)
    assert TG.same_bits(why, TG.reason(rule, B, None, None, None, ahead)) and not why.any() and not mask.any()
    assert not SC.differing(SC.snapshot(s), before, np.ones(B, bool))
    moved = np.arange(B) % 2 == 1
    x0 = s.get_initial_state()
    x0[moved, 1] += 0.3
    s.set_initial_state(x0)
    ahead = s.mpc_track(L, 1, log=False)["stats"][:, 0]
    print("lookahead violations, moved:", ahead["violation"][moved].min(), ahead["violation"][moved].max(), "others:",
          ahead["violation"][~moved].max())
    age = (np.arange(B) % 3).astype(np.int32)
    mask, why = s.mpc_trigger(rule, age=age)
    assert TG.same_bits(why, TG.reason(rule, B, None, age, None, ahead))
    assert np.array_equal(why == TG.AHEAD, moved) and np.array_equal(mask, moved)
    # with the bounds the lookahead clips as altro_mpc_track does
    ahead = s.mpc_track(L, 1, u_lo=LO, u_hi=HI, log=False)["stats"][:, 0]
    _, why = s.mpc_trigger(rule, u_lo=LO, u_hi=HI)
    assert TG.same_bits(why, TG.reason(rule, B, None, None, None, ahead))
    s.close()


def test_lookahead_in_the_run(A, P, hip_make):
    """A pulse of 0.3 in y on the odd instances at the last knot of cycle 0 (the state cycle 1 starts from lies inside the
    circle), no other criterion but the age (4): AHEAD occurs as the only bit, asserted on the composed loop, and the run is
    that loop bit for bit."""
    B, cycles, shift = 6, 4, 2
    ref_h, run_h = _turn90_beside_a_circle(P, hip_make, B), _turn90_beside_a_circle(P, hip_make, B)
    rule = TG.rule_dict(max_age=4, lookahead=6, ahead_tol=ref_h.get_options().constraint_tolerance)
    w = np.zeros((cycles, B, shift, 3))
    w[0, 1::2, shift - 1, 1] = 0.3
    ref = TG.composed_loop(ref_h, cycles, shift, rule, w)
    print("reasons\n", ref["reason"])
    assert (ref["reason"][1::2, 1] == TG.AHEAD).all() and (ref["reason"][::2, 1:] == 0).all()
    got = run_h.mpc_run_triggered(cycles, shift, rule, w=w)
    _compare_runs(got, ref, "lookahead")
    assert not SC.differing(SC.snapshot(run_h), SC.snapshot(ref_h), np.ones(B, bool))
    ref_h.close()
    run_h.close()


# ---- 6. refusals on the device ---------------------------------------------------------------------------------------------
def test_refusals_on_the_device(A, P, hip_make):
    """After each refusal the handle's mask state is as it was, and a following plain solve gives the bits of a fresh handle."""
    B = 6
    ok = TG.rule_dict(max_age=2, dx_tol=DX_TOL)

    def refused(call, status, word):
        with pytest.raises(A.AltroError) as e:
            call()
        assert _status_of(e) == status and word in str(e.value), str(e.value)

    def solves_like_fresh(s, prepare=lambda h: None):
        fresh = _build(A, P, hip_make, "turn90_f64", B)
        prepare(fresh)
        fresh.solve()
        s.solve()
        assert not SC.differing(SC.snapshot(s), SC.snapshot(fresh), np.ones(B, bool))
        fresh.close()
    # a handle with a mask set: the run refuses, the mask stays
    s = _build(A, P, hip_make, "turn90_f64", B)
    mask = np.arange(B) % 2 == 0
    s.set_solve_mask(mask)
    refused(lambda: s.mpc_run_triggered(2, 2, ok), A.UNSUPPORTED, "mask")
    assert np.array_equal(s.get_solve_mask(), mask)
    s.mpc_trigger(ok)  # (the evaluation does not mind a mask, and leaves it)
    assert np.array_equal(s.get_solve_mask(), mask)
    s.set_solve_mask(None)
    solves_like_fresh(s)
    s.close()
    # cost-to-go records
    s = _build(A, P, hip_make, "turn90_f64", B)
    s.set_record_ctg(True)
    refused(lambda: s.mpc_run_triggered(2, 2, ok), A.UNSUPPORTED, "cost-to-go")
    refused(lambda: s.mpc_trigger(ok), A.UNSUPPORTED, "cost-to-go")
    assert s.get_solve_mask().all()
    solves_like_fresh(s, lambda h: h.set_record_ctg(True))
    s.close()
    # per-knot steps
    steps = np.full(N, 0.125, dtype=np.float32)
    s = _build(A, P, hip_make, "turn90_f64", B)
    s.set_steps(steps)
    refused(lambda: s.mpc_run_triggered(2, 2, ok), A.UNSUPPORTED, "per-knot")
    refused(lambda: s.mpc_trigger(ok), A.UNSUPPORTED, "per-knot")
    assert s.get_solve_mask().all()
    solves_like_fresh(s, lambda h: h.set_steps(steps))
    s.close()
    # the age bound: (5 - 1) 5 + 5 = 25 > 24
    s = _build(A, P, hip_make, "turn90_f64", B)
    refused(lambda: s.mpc_run_triggered(2, 5, TG.rule_dict(max_age=5)), A.INVALID_ARG, "held tail")
    # no gains yet, with a lookahead
    refused(lambda: s.mpc_trigger(TG.rule_dict(max_age=2, lookahead=3, ahead_tol=1e-4)), A.NOT_READY, "gains")
    assert s.get_solve_mask().all()
    solves_like_fresh(s)
    s.close()


# ---- 7. the facade ---------------------------------------------------------------------------------------------------------
def test_facade_gives_the_c_calls_bits(A, P, hip_make, tmp_path):
    """tests/cpp/trigger_facade_driver.cpp: Solve, TrackClosedLoop, EvaluateTrigger, RunTriggered on B = 6, printing hexadecimal
    floats; the C calls on the same inputs give the same bits."""
    B, cycles, shift, max_age = 6, 5, 2, 3
    exe = str(tmp_path / "trigger_facade_driver")
    csrc = os.path.join(ROOT, "altro-cpp_amd", "csrc")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "cpp", "trigger_facade_driver.cpp"), "-L" + csrc, "-laltro_hip", "-Wl,-rpath," + csrc,
                        "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    x0 = np.zeros((B, 3))
    x0[:, 0] = 0.02 * np.arange(B)
    x0[:, 2] = -0.01 * np.arange(B)
    w = TG.pulses(cycles, B, shift, 3, 10 * DX_TOL)
    w[0, 0, 1, 0] = 3 * DX_TOL  # (so that the evaluation behind the first tracked segment sees a deviation too)
    age = np.arange(B) % 4
    path = str(tmp_path / "inputs.bin")
    np.concatenate([x0.ravel(), w.ravel(), age.astype(np.float64)]).tofile(path)
    r = subprocess.run([exe, path, str(B), str(N), str(cycles), str(shift), str(max_age), repr(DX_TOL)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if f[0] in ("X_cl", "U_cl"):
            rows[f[0]] = np.array([float.fromhex(v) for v in f[1:]])
        elif f[0] == "track":
            rows[f[0]] = [int(v) if i % 6 < 2 else float.fromhex(v) for i, v in enumerate(f[1:])]
        else:
            rows[f[0]] = np.array([int(v) for v in f[1:]], dtype=np.int32)
    s = P.unicycle_turn90(hip_make, batch=B, N=N)
    s.set_initial_state(x0)
    rule = TG.rule_dict(max_age=max_age, dx_tol=DX_TOL, on_unsolved=1)
    s.solve()
    assert rows["solved"][0] == s.get_stats()["status"][0]
    seg = s.mpc_track(shift, 1, w=w[0][:, None], u_lo=LO, u_hi=HI, log=False)["stats"][:, 0]
    mask, why = s.mpc_trigger(rule, tracked=seg, age=age, u_lo=LO, u_hi=HI)
    assert np.array_equal(rows["mask"] != 0, mask) and TG.same_bits(rows["why"], why)
    assert why.any() and not why.all()
    out = s.mpc_run_triggered(cycles, shift, rule, w=w, u_lo=LO, u_hi=HI)
    for key in ("X_cl", "U_cl"):
        assert TG.same_bits(rows[key], out[key].ravel()), key
    for key in ("iterations", "status", "reason"):
        assert TG.same_bits(rows[key], out[key].ravel()), key
    track = np.zeros(B * cycles, dtype=A.TRACK_STATS_DTYPE)
    for i in range(B * cycles):
        track[i] = tuple(rows["track"][6 * i:6 * i + 6])
    for field in track.dtype.names:
        assert TG.same_bits(np.ascontiguousarray(track[field]), np.ascontiguousarray(out["track"].ravel()[field])), field
    assert (out["reason"] == 0).any() and rows["after"][0] == s.get_stats()["status"][0]
    s.close()
