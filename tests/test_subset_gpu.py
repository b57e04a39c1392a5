"""The solve mask and sequential team rounds on the device (include/altro_subset.h).  The yardstick of a masked solve is a
TWIN handle in the same state that solves without a mask: masked-in instances equal the twin's bit for bit, masked-out
instances equal their own snapshot from before the solve.  Every problem has N = 24."""
import ctypes
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ledger
import _subset_common as SC
import _team_common as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = SC.N
RTOL, ATOL = 1e-7, 1e-9  # tests/test_knot_params_gpu.py::_compare_with_oracle
# 6, 65: the tail at once (65: a column behind lane 63); 700: where an unmasked solve takes the device-side loop; 2100: four chains
SIZES = (6, 65, 700, 2100)
CASES = [(B, name) for B in SIZES for name in SC.patterns(B)]


def _hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("the solver library has not loaded a HIP runtime")


class DeviceBytes:
    """device memory holding the given bytes (hipMalloc / hipMemcpy through ctypes)"""

    def __init__(self, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        self.hip = _hip_runtime()
        p = ctypes.c_void_p()
        assert self.hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(max(data.size, 1))) == 0
        self.ptr = p.value
        assert self.hip.hipMemcpy(ctypes.c_void_p(self.ptr), data.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(data.size),
                                  ctypes.c_int(1)) == 0  # host to device

    def free(self):
        self.hip.hipFree(ctypes.c_void_p(self.ptr))


def _second_guess(s):
    """a state that is no solve's start and no zeros: the solved handle gets another initial guess"""
    s.set_trajectory(None, np.tile(np.array([0.2, 0.05]), (s.N, 1)))


def _pair(P, make, B, build=None, history=False):
    """(handle, twin) in the same state: both solved once without a mask, then given the same second guess"""
    build = build or (lambda mk: P.batch_turn90(mk, B, N=N))
    pair = []
    for _ in range(2):
        s = build(make)
        if history:
            s.set_record_history(64)
        s.solve()
        _second_guess(s)
        pair.append(s)
    return pair


def _check_masked(s, t, mask, solve=lambda h: h.solve(), history=False, label=""):
    """solve `s` under `mask` and the twin `t` without one; assert the contract; returns the two timings"""
    mask = np.asarray(mask, dtype=bool)
    before = SC.snapshot(s, history)
    s.set_solve_mask(mask)
    assert (s.get_solve_mask() == mask).all()
    solve(s)
    solve(t)
    got, twin = SC.snapshot(s, history), SC.snapshot(t, history)
    bad_in, bad_out = SC.differing(got, twin, mask), SC.differing(got, before, ~mask)
    print(f"{label}: {int(mask.sum())} of {mask.size} masked in; differ from the twin: {bad_in}; changed though masked out: {bad_out}")
    assert not bad_in, bad_in
    assert not bad_out, bad_out
    if mask.any():
        assert SC.differing(got, before, mask), "the masked solve changed nothing: the test state is a fixed point"
    ts, tt = s.get_timing(), t.get_timing()
    st = t.get_stats()
    assert ts["instance_iterations"] == int(st["iterations_total"][mask].sum())
    return ts, tt


# ---- 1. every size, every pattern ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,name", CASES, ids=[f"B{B}_{name}" for B, name in CASES])
def test_masked_solve_against_the_twin(A, P, hip_make, B, name):
    s, t = _pair(P, hip_make, B, history=B <= 65)
    mask = SC.patterns(B)[name]
    ts, tt = _check_masked(s, t, mask, history=B <= 65, label=f"B{B} {name}")
    print(f"launches masked {ts['launches']} twin {tt['launches']}")
    if name == "ones" and B == 6:
        assert ts["launches"] == tt["launches"], (ts["launches"], tt["launches"])
    if name == "zeros":
        assert ts["launches"] == 0
    if name == "spread40":  # fits the tail from sweep 0: begin, merge, the persistent kernel
        assert ts["sweep_launches"] == 0 and ts["launches"] <= 3, ts
    s.close()
    t.close()


def _launches_at_2100(P, make, masked):
    s = P.batch_turn90(make, 2100, N=N)
    s.solve()
    _second_guess(s)
    if masked:
        s.set_solve_mask(np.ones(2100, bool))
    s.solve()
    t = s.get_timing()
    s.close()
    return t["launches"], t["sweep_launches"], t["sweeps"]


def test_full_mask_launches_what_no_mask_launches_on_four_chains(A, P, hip_make, monkeypatch):
    """B = 2100, all ones.  Only the first large handle of a process gets chains of its own, so the two handles of a pair do not
    launch alike whatever their masks; here each handle lives alone, one after the other.
    Under the default policy the launch count of a four-chain solve is not a function of its inputs: the host hands over to the
    persistent kernel when the counts it has HEARD OF from the four chains fall below the threshold, and a chain may have run
    one sweep more by then.  Measured on an MI355X, eight fresh handles each: without a mask 147 launches seven times and 150
    once, under a full mask 147 four times and 150 four times; `sweeps`, the longest chain of iterations, 115 every time.  So
    launch-for-launch equality is asserted where the count is a function of the inputs -- the same four chains without the
    hand-over (ALTRO_HIP_NO_FUSED_SWEEP, read when the engine is made): 1066 launches either way -- and under the default policy
    the figure that is one, `sweeps`, must agree."""
    default = [_launches_at_2100(P, hip_make, masked) for masked in (True, False)]
    monkeypatch.setenv("ALTRO_HIP_NO_FUSED_SWEEP", "1")
    paced = [_launches_at_2100(P, hip_make, masked) for masked in (True, False)]
    print(f"(launches, sweep launches, sweeps) full mask / no mask: default policy {default}, without the hand-over {paced}")
    assert paced[0] == paced[1], paced
    assert paced[0][1] > 4 * 48  # (four chains ran: one chain's sweeps alone would be a quarter of this)
    assert default[0][2] == default[1][2], default


# ---- 2. the other paths, once each at B = 65, every other instance ---------------------------------------------------------
def _team_build(P):
    def build(mk):
        s = P.team_ring(mk, 13, 5, N=N)
        return s
    return build


OTHER = ["tripleint", "team", "f32", "warm", "ilqr", "async"]


@pytest.mark.parametrize("path", OTHER)
def test_other_paths(A, P, hip_make, path):
    B = 65
    mask = np.arange(B) % 2 == 0
    solve = lambda h: h.solve()  # noqa: E731
    if path == "tripleint":
        s, t = _pair(P, hip_make, B, lambda mk: P.batch_triple_integrator(mk, B, N=N))
    elif path == "team":
        s, t = _pair(P, hip_make, B, _team_build(P))
        for h in (s, t):  # the uncoupled plans are gone with the second guess: couple the plans of the first solve's successor
            h.solve()
            h.team_fill_tracks(5, h.team_circle, h.team_radius)
    elif path == "f32":
        s, t = _pair(P, hip_make, B, lambda mk: P.batch_turn90(mk, B, N=N, dtype=A.F32))
    else:
        s, t = _pair(P, hip_make, B)
    if path == "warm":
        for h in (s, t):
            h.solve()
            h.set_options(reset_duals=0)
            h.mpc_advance(2)
    if path == "ilqr":
        solve = lambda h: h.solve_ilqr()  # noqa: E731
    if path == "async":
        def solve(h):
            h.solve_async()
            h.wait()
    _check_masked(s, t, mask, solve, label=path)
    s.close()
    t.close()


# ---- 3. poisoned shadow columns ---------------------------------------------------------------------------------------------
def _spread40_solve(A, P, make):
    s, t = _pair(P, make, 2100)
    s.set_solve_mask(SC.patterns(2100)["spread40"])
    s.solve()
    out = {k: v for k, v in SC.snapshot(s).items()}
    s.close()
    t.close()
    return out


_POISON_SCRIPT = """
import importlib, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import __graft_entry__ as graft
A = graft.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
import test_subset_gpu as T
np.savez(sys.argv[1], **T._spread40_solve(A, P, P.make_hip))
"""


def test_masked_solve_needs_nothing_behind_the_batch(A, P, hip_make, tmp_path):
    """B = 2100 with the 40-instance mask in a fresh process with ALTRO_HIP_DEBUG_POISON: the same bits."""
    ref = _spread40_solve(A, P, hip_make)
    out = str(tmp_path / "poisoned.npz")
    subprocess.run([sys.executable, "-c", _POISON_SCRIPT % (ROOT, os.path.join(ROOT, "tests")), out], check=True,
                   env=dict(os.environ, ALTRO_HIP_DEBUG_POISON="1"), timeout=600)
    got = dict(np.load(out))
    assert not SC.differing(ref, got, np.ones(2100, bool))


# ---- 4. the setters -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [65, 2100])
def test_host_and_device_setters_agree(A, P, hip_make, B):
    s, t = _pair(P, hip_make, B)
    mask = np.random.default_rng(B).random(B) < 0.3
    raw = np.where(mask, 1 + np.arange(B) % 250, 0).astype(np.uint8)  # any non-zero byte counts
    dev = DeviceBytes(raw)
    s.set_solve_mask(mask)
    t.set_solve_mask_device(dev.ptr)
    dev.free()  # (the bytes were copied)
    assert (s.get_solve_mask() == mask).all() and (t.get_solve_mask() == mask).all()
    s.solve()
    t.solve()
    assert not SC.differing(SC.snapshot(s), SC.snapshot(t), np.ones(B, bool))
    s.close()
    t.close()


def test_mask_survives_setters_and_goes_when_cleared(A, P, hip_make):
    B = 65
    s, t = _pair(P, hip_make, B)
    mask = np.arange(B) % 3 == 1
    s.set_solve_mask(mask)
    _second_guess(s)
    s.solve()
    s.mpc_advance(2)
    t.solve()
    t.mpc_advance(2)
    assert (s.get_solve_mask() == mask).all()
    with pytest.raises(A.AltroError):  # the definition is fixed once it is on the device; the refusal leaves the mask alone
        s.add_goal_constraint(N, np.zeros(3))
    assert (s.get_solve_mask() == mask).all()
    before = SC.snapshot(s)
    s.solve()
    assert not SC.differing(SC.snapshot(s), before, ~mask)
    assert SC.differing(SC.snapshot(s), before, mask)
    s.set_solve_mask(None)
    assert s.get_solve_mask().all()
    before = SC.snapshot(s)
    s.solve()
    assert len(SC.differing(SC.snapshot(s), before, ~mask)) > 0
    s.close()
    t.close()


def test_masked_solve_refuses_cost_to_go_records(A, P, hip_make):
    s = P.batch_turn90(hip_make, 6, N=N)
    s.set_record_ctg(True)
    s.solve()
    s.set_solve_mask(np.arange(6) < 3)
    before = SC.snapshot(s)
    with pytest.raises(A.AltroError, match=r"\(%d\).*cost-to-go" % A.UNSUPPORTED):
        s.solve()
    assert not SC.differing(SC.snapshot(s), before, np.ones(6, bool))
    s.set_solve_mask(None)
    s.solve()
    s.close()


def test_not_ready_while_an_asynchronous_solve_is_in_flight(A, P, hip_make):
    s = P.team_ring(hip_make, 3, 2, N=N)
    s.solve()
    s.solve_async()
    calls = [lambda: s.set_solve_mask(np.ones(6, bool)), lambda: s.set_solve_mask_device(64), lambda: s.get_solve_mask(),
             lambda: s.team_solve_sequential(2, s.team_circle, s.team_radius, 1)]
    try:
        for call in calls:
            with pytest.raises(A.AltroError, match=r"\(%d\)" % A.NOT_READY):
                call()
    finally:
        s.wait()
    s.close()


# ---- 5. sequential team rounds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,Ag", [(3, 2), (2, 3), (65, 5), (700, 3)], ids=["B6_A2", "B6_A3", "B325_A5", "B2100_A3"])
def test_sequential_is_the_callers_loop(A, P, hip_make, T, Ag):
    B = T * Ag
    pair = []
    for _ in range(2):
        s = P.team_ring(hip_make, T, Ag, N=N)
        s.solve()
        pair.append(s)
    s, t = pair
    own = np.arange(B) % 4 != 3  # the caller's own mask: back afterwards
    s.set_solve_mask(own)
    t.set_solve_mask(own)
    s.team_solve_sequential(Ag, s.team_circle, s.team_radius, 1)
    SC.sequential_loop(t, Ag, t.team_circle, t.team_radius, 1)
    assert (s.get_solve_mask() == own).all()
    assert not SC.differing(SC.snapshot(s), SC.snapshot(t), np.ones(B, bool))
    s.close()
    t.close()


@pytest.mark.parametrize("T,Ag", [(3, 2), (2, 3)], ids=["T3_A2", "T2_A3"])
def test_every_turn_against_the_oracle(A, P, oracle_make, hip_make, T, Ag):
    """Each turn the oracle gets the device's own track rows and pre-solve controls, and solves everyone; the rows of the
    turn's agents must agree: statuses and iteration counts exact, X and U to 1e-7 relative + 1e-9.  Afterwards the behaviour
    bars of tests/test_subset_oracle.py hold on the device's own plans."""
    B = T * Ag
    g = P.team_ring(hip_make, T, Ag, N=N)
    idx, rad = g.team_circle, g.team_radius
    g.solve()
    unc = TC.distance_clearance(g.get_trajectory()[0], Ag, rad, 1, N)
    for a in range(Ag):
        turn = np.arange(B) % Ag == a
        g.team_fill_tracks(Ag, idx, rad, A.TEAM_ALL, 1.0)
        rows = np.zeros((B, N + 1, 3 * (Ag - 1)))
        rows[:, 1:N] = g.get_knot_params(idx)
        o = P.team_ring(oracle_make, T, Ag, N=N, per_knot_track=rows, U=g.get_trajectory()[1])
        o.solve()
        g.set_solve_mask(turn)
        g.solve()
        so, sg = o.get_stats(), g.get_stats()
        for f in ("status", "iterations_total", "iterations_outer"):
            assert (so[f][turn] == sg[f][turn]).all(), (a, f, so[f], sg[f])
        Xo, Uo = o.get_trajectory()
        Xg, Ug = g.get_trajectory()
        _ledger.close(Xg[turn], Xo[turn], RTOL, ATOL, "X")
        _ledger.close(Ug[turn], Uo[turn], RTOL, ATOL, "U")
        o.close()
    cpl = TC.distance_clearance(g.get_trajectory()[0], Ag, rad, 1, N)
    st = g.get_stats()
    print(f"T{T} A{Ag}: uncoupled {unc}, after one sequential sweep {cpl}, statuses {np.unique(st['status'])}")
    assert (st["status"] == A.SOLVED).all(), st["status"]
    assert (cpl >= TC.COUPLED_BAR).all(), cpl
    g.close()


def test_sequential_sweep_stops_collisions_T2_A5(A, P, hip_make):
    """the third behaviour case of tests/test_subset_oracle.py on the device's own plans, through the one call"""
    T, Ag = 2, 5
    s = P.team_ring(hip_make, T, Ag, N=N)
    s.solve()
    s.team_solve_sequential(Ag, s.team_circle, s.team_radius, 1)
    cpl = TC.distance_clearance(s.get_trajectory()[0], Ag, s.team_radius, 1, N)
    st = s.get_stats()
    print(f"T2 A5: after one sequential sweep {cpl}, statuses {np.unique(st['status'])}")
    assert (st["status"] == A.SOLVED).all(), st["status"]
    assert (cpl >= TC.COUPLED_BAR).all(), cpl
    s.close()
