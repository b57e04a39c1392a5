"""The knot-routed kernels (Engine::KnotRouted: k_expansions_trk, k_forward_trk, k_knot_costs_trk, k_mpc_track_trk, fed by
k_ref_pack, k_ref_terms<T, n, m>, k_knot_params, moved by k_mpc_advance) on every shape of the model matrix of
tests/test_model_shapes_gpu.py, and together with multi-start.

The record layouts -- RefPathRecord(n, m) = (n + m + 1) & ~1, RefTermRecord(n, m) = (n + m + 2) & ~1, the knot-parameter
record with elements at odd offsets when a constraint's width is odd -- depend on n and m; tests/test_tracking_gpu.py and
tests/test_knot_params_gpu.py run them at (3,2), (6,2) and (4,1).  Here: n + m odd and even (a padding element or none), n = 1
(the two-element path record), m > n, n m >= 12, and the fp32 record strides.

The problem is _knot_shapes_common.chain_tracking (N = 20, path and track of N + 1 + 8 = 29 rows, batch 12 unless stated):
tests/models/shape_chain.hpp following its own rollout under symmetric, not diagonal, Q and R and a control bound that tightens
along the track.  On the CPU oracle (offsets 0 and 7, all ten shapes): every instance SOLVED, 6 to 14 iterations, 2 to 5
outer, violation <= 1e-4, the bound reached by every instance.  The multi-start tests run problems.moving_obstacles as six
problems x four adjacent starts.  Every comparison lands in the ledger (tests/_ledger.py) next to its bar; the bars are the
project's own, cited where they are used."""
import numpy as np
import pytest

import _knot_shapes_common as KS
import _ledger
import _mpc_common as M
import _multistart_common as MS
from test_model_shapes_gpu import COOP, F32_SHAPES, MFMA4, MFMA16, SHAPES, _F32_BARS, chain_goals, chain_rk4, kind_of, oracle_of
from test_tracking_gpu import DeviceArray, _host_terms, _same, _state

pytestmark = pytest.mark.gpu

N, ROWS, B = 20, 20 + 1 + 8, 12
# the project's fp64 bars -- trajectories (tests/test_tracking_gpu.py::test_solve_against_the_oracle)
RTOL, ATOL = 1e-7, 1e-9
# one shape per backward kernel: 4 x 4 MFMA, 16 x 16 MFMA, cooperative, VALU
PER_KERNEL = [(2, 2), (5, 3), (13, 2), (3, 5)]
assert PER_KERNEL[0] in MFMA4 and PER_KERNEL[1] in MFMA16 and PER_KERNEL[2] in COOP and PER_KERNEL[3] not in MFMA4 + MFMA16 + COOP


def ids(shapes):
    return [f"{n}_{m}" for n, m in shapes]


def _pair(A, hip_make, n, m, **kw):
    """-> (oracle handle with one cost and one bound per knot, device handle with the tracking cost and the knot constraint)"""
    kind = kind_of(A, n, m)
    return (KS.chain_tracking(A, oracle_of(A, n, m), kind, n, m, per_knot=True, **kw),
            KS.chain_tracking(A, hip_make, kind, n, m, **kw))


def _terms_of(n, m, Xw, Uw, Q=None, R=None, Qf=None):
    """_host_terms over a window [B][N + 1][.]: Q, R on [0, N), Qf and R = 0 on knot N"""
    Q0, R0, Qf0 = KS.chain_costs(n, m)
    Q, R, Qf = Q0 if Q is None else Q, R0 if R is None else R, Qf0 if Qf is None else Qf
    q, r, c = _host_terms(Q, R, Xw[:, :-1], Uw[:, :-1])
    qf, rf, cf = _host_terms(Qf, R * 0, Xw[:, -1], Uw[:, -1])
    return (np.concatenate([q, qf[:, None]], axis=1), np.concatenate([r, rf[:, None]], axis=1), np.concatenate([c, cf[:, None]], axis=1))


def _same_bytes(got, want, what):
    want = np.ascontiguousarray(np.broadcast_to(want, got.shape))
    assert got.tobytes() == want.tobytes(), (what, np.argwhere(got != want)[:4].tolist())


def _same_terms(got, want, what):
    for name, x, y in zip("qrc", got, want):
        _same_bytes(x, y, (what, name))


# Bars of the whole solves: (X, U: relative, absolute; cost: relative; violation: relative, absolute).
# TIGHT is what tests/test_tracking_gpu.py::test_solve_against_the_oracle holds, and what every quantity of every case holds
# here unless _SOLVE_BARS names it.
TIGHT = dict(X=(RTOL, ATOL), U=(RTOL, ATOL), cost=(1e-10, 0.0), violation=(1e-7, 1e-12))
MARGIN = 10  # of a bar over the measurement it stands on: the margin of tests/test_model_shapes_gpu.py's _AL_BARS


def _bar(figure):
    """MARGIN x figure, rounded up to 1 / 2 / 5 of its decade (as _AL_BARS and _F32_BARS are)"""
    x = MARGIN * figure
    e = np.floor(np.log10(x))
    for lead in (1, 2, 5, 10):
        if x <= lead * 10.0 ** e * (1 + 1e-9):
            return float(f"{lead}e{int(e)}") if lead < 10 else float(f"1e{int(e) + 1}")


# The quantities that miss TIGHT on the MI355X with the schedule exact, each with its own bar.  On X, on every case, and on
# every other quantity the GPU holds TIGHT (the cases (1,1) offset 0, (13,2) offset 7 and (6,5) offset 7 among them: U within
# 5e-11, cost within 3e-14).  The misses are one step more or less of 1e-8 .. 1e-7 at the end of a converged solve: the last
# line search accepts its step on a ratio of two differences at rounding level.  The ORACLE ALONE does the same, which is
# what the bars stand on.  Per entry:
#   gpu   what the MI355X measures against the oracle (profiles/r06_parity_errors.json; absolute, the cost relative)
#   ulp   the oracle against itself with one input moved by one unit in the last place (_knot_shapes_common.ULPS: x0, Q, R,
#         the path, the bound, each alone; the maximum; schedule unmoved, K within 4e-13 norm-wise), measured on the CPU
#   step  the oracle against itself with the host's costs and path built from the fp32-rounded step float(np.float32(0.05))
#         (what every handle here takes) and from 0.05 (the library's own step is a 32-bit float either way); schedule unmoved
#   bar   _bar(ulp): the absolute part of the bar (for the cost: the relative bar); the relative parts stay TIGHT's
# `step` moves the problem by 1.5e-8 relative, not by a rounding: it shows how far the minimum itself goes (X 2e-9 .. 2e-8,
# U up to 1.5e-7, cost 6e-9 .. 1.5e-7, on the cases that hold TIGHT as on these; the violation of (5,3) offset 7 not at all).
# It stands beside the bars; they stand on `ulp`, what rounding alone does to the reference, which is what separates the GPU
# from it (compare the columns gpu and ulp).  The third measurement, the ordinary path of the same shape on the
# same problem, cannot be made: per knot this problem has N + 1 costs and N bounds, 21 knot classes, and the library refuses
# more than kMaxClasses = 8 ("too many distinct knot-point classes", altro_problem.hpp).  What stands in for it: with a
# constant path and constant tracks the knot-routed and the ordinary path agree byte for byte on every shape (test 3), and
# the ordinary path against the oracle on its own problem shows the same steps (_AL_BARS: U 1e-5 at (7,3), (9,1)).
# test_the_bars_stand_on_the_oracles_own_answer repeats `ulp` and `step` on every run and holds them to this table.
#   (shape, offset, N):            quantity:       gpu       ulp       step      bar
_SOLVE_BARS = {
    ((2, 2), 7, 20): dict(U=(1.0e-08, 2.4e-08, 1.9e-08, 5e-07), violation=(3.9e-10, 9.7e-10, 3.9e-10, 1e-08)),
    ((5, 3), 0, 20): dict(U=(1.7e-08, 1.7e-08, 1.0e-07, 2e-07), violation=(5.7e-10, 5.7e-10, 5.7e-10, 1e-08)),
    ((5, 3), 7, 20): dict(U=(4.7e-08, 4.7e-08, 5.2e-08, 5e-07), cost=(2.5e-09, 2.5e-09, 2.3e-08, 5e-08),
                          violation=(5.2e-10, 7.6e-10, 5.4e-14, 1e-08)),
    ((6, 5), 0, 20): dict(U=(2.1e-08, 2.1e-08, 2.9e-08, 5e-07), cost=(6.2e-10, 6.2e-10, 1.5e-07, 1e-08)),
    ((7, 3), 0, 20): dict(violation=(3.5e-12, 6.0e-12, 2.8e-12, 1e-10)),
    ((7, 3), 7, 20): dict(U=(5.1e-08, 6.2e-08, 7.3e-08, 1e-06), violation=(1.0e-09, 1.0e-09, 1.0e-09, 1e-08)),
    ((3, 5), 0, 20): dict(U=(2.1e-08, 4.1e-08, 3.9e-08, 5e-07), violation=(1.2e-11, 2.3e-11, 1.7e-11, 5e-10)),
    ((3, 5), 7, 20): dict(U=(6.3e-08, 6.3e-08, 4.8e-08, 1e-06), violation=(1.9e-10, 1.9e-10, 1.5e-10, 2e-09)),
    ((5, 3), 0, 33): dict(U=(2.8e-08, 6.3e-08, 1.5e-07, 1e-06), cost=(1.0e-09, 3.1e-09, 4.1e-08, 5e-08)),  # test 6, batch 8
}
assert all(row[3] == _bar(row[1]) for case in _SOLVE_BARS.values() for row in case.values())


def _bars(shape, offset, horizon=N):
    bars = dict(TIGHT)
    for name, row in _SOLVE_BARS.get((shape, offset, horizon), {}).items():
        bars[name] = (row[3], 0.0) if name == "cost" else (TIGHT[name][0], row[3])
    return bars


def _all(checks):
    """every comparison is made and lands in the ledger before the first one that missed its bar is reported"""
    missed = []
    for check in checks:
        try:
            check()
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, missed


def _against_the_oracle(A, o, g, tag, bars=TIGHT, solve="solve"):
    """Status, total and outer iterations exact; X, U, the cost and the violation within ``bars``."""
    getattr(o, solve)()
    getattr(g, solve)()
    so, sg = o.get_stats(), g.get_stats()
    print(f"{tag}: iterations {so['iterations_total'].min()} .. {so['iterations_total'].max()}, outer {so['iterations_outer'].min()} .. "
          f"{so['iterations_outer'].max()}, statuses {np.unique(so['status'])}")
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (tag, f, np.flatnonzero(so[f] != sg[f])[:8])
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    for name, got, want in (("X", Xg, Xo), ("U", Ug, Uo), ("cost", sg["cost"], so["cost"]), ("violation", sg["violation"], so["violation"])):
        if bars[name] != TIGHT[name]:  # (an entry of _SOLVE_BARS is there because TIGHT is missed: say so where it is not)
            rtol, atol = TIGHT[name]
            miss = (np.abs(got - want) > atol + rtol * np.maximum(np.abs(got), np.abs(want))).sum()
            print(f"{tag}: {name} misses TIGHT on {miss} elements, max |difference| {np.abs(got - want).max():.2e}")
    _all([lambda: _ledger.close(Xg, Xo, *bars["X"], f"{tag}: X"),
          lambda: _ledger.close(Ug, Uo, *bars["U"], f"{tag}: U"),
          lambda: _ledger.close(sg["cost"], so["cost"], *bars["cost"], f"{tag}: stat cost"),
          lambda: _ledger.close(sg["violation"], so["violation"], *bars["violation"], f"{tag}: stat violation")])
    return so, Uo


def _oracle_alone(A, n, m, **kw):
    o = KS.chain_tracking(A, oracle_of(A, n, m), kind_of(A, n, m), n, m, per_knot=True, **kw)
    o.solve()
    st = o.get_stats()
    out = dict(zip(("X", "U"), o.get_trajectory()), cost=st["cost"].copy(), violation=st["violation"].copy(),
               schedule=np.stack([st["status"], st["iterations_total"], st["iterations_outer"]]))
    o.close()
    return out


def _moved(a, b):
    """|dX|, |dU|, |dcost| / cost, |dviolation| between two answers of the oracle; its schedule must not move"""
    assert np.array_equal(a["schedule"], b["schedule"])
    return dict(X=np.abs(a["X"] - b["X"]).max(), U=np.abs(a["U"] - b["U"]).max(), cost=np.abs(a["cost"] / b["cost"] - 1).max(),
                violation=np.abs(a["violation"] - b["violation"]).max())


@pytest.mark.parametrize("shape,offset,horizon", list(_SOLVE_BARS), ids=[f"{n}_{m}-o{o}-N{h}" for (n, m), o, h in _SOLVE_BARS])
def test_the_bars_stand_on_the_oracles_own_answer(A, shape, offset, horizon):
    """The two measurements behind _SOLVE_BARS, on the oracle alone (CPU work: no kernel runs here): `ulp` and `step` of
    every entry are measured again and agree with the table within a factor of 2 either way, so that the bar of an entry,
    _bar(ulp), stays between 5 and 100 times what the oracle does on its own."""
    n, m = shape
    kw = dict(offset=offset) if horizon == N else dict(offset=offset, batch=8, N=horizon, rows=horizon + 1)
    base = _oracle_alone(A, n, m, **kw)
    ulp = dict.fromkeys(("X", "U", "cost", "violation"), 0.0)
    for u in KS.ULPS:
        for name, v in _moved(_oracle_alone(A, n, m, ulp=u, **kw), base).items():
            ulp[name] = max(ulp[name], v)
    step = _moved(_oracle_alone(A, n, m, host_step=0.05, **kw), base)
    tag = f"{n}_{m} offset {offset}" + (f" N {horizon}" if horizon != N else "")
    for name, (_, t_ulp, t_step, bar) in _SOLVE_BARS[(shape, offset, horizon)].items():
        _ledger.record(f"{tag}: oracle against itself, one ulp: {name}", ulp[name], ulp[name], ulp[name] / bar, 0.0, bar,
                       note="max over _knot_shapes_common.ULPS")
        _ledger.record(f"{tag}: oracle against itself, un-rounded step: {name}", step[name], step[name], step[name] / bar, 0.0, bar)
        assert t_ulp / 2 <= ulp[name] <= t_ulp * 2, (name, ulp[name], t_ulp)
        assert t_step / 2 <= step[name] <= t_step * 2, (name, step[name], t_step)


# ---- 1. the whole solve against the oracle ------------------------------------------------------------------------------------------
_SOLVE_CASES = [(s, B, o) for s in SHAPES for o in (0, 7)] + [(s, 70, o) for s in PER_KERNEL for o in (0, 7)]


@pytest.mark.parametrize("shape,batch,offset", _SOLVE_CASES, ids=[f"{n}_{m}-b{b}-o{o}" for (n, m), b, o in _SOLVE_CASES])
def test_solve_against_the_oracle(A, hip_make, shape, batch, offset):
    """All ten shapes at offsets 0 and 7; batch 70 (past one wavefront, the second partly filled; the parameters repeat with
    b mod 5, so the bars are those of batch 12) for one shape per backward kernel.  Bars: TIGHT, but for the quantities
    _SOLVE_BARS names.  On the oracle every instance ends SOLVED and max |U| reaches the smallest bound of the instance's
    window: the problem has not gone slack."""
    n, m = shape
    o, g = _pair(A, hip_make, n, m, batch=batch, offset=offset)
    so, Uo = _against_the_oracle(A, o, g, f"{n}_{m} batch {batch} offset {offset}" if batch != B else f"{n}_{m} offset {offset}",
                                 _bars(shape, offset))
    assert (so["status"] == A.SOLVED).all()
    ub = KS.window(KS.chain_bound(m, batch, ROWS)[0][:, :, None], offset, np.arange(N))[:, :, 0]
    assert (np.abs(Uo).max(axis=(1, 2)) >= ub.min(axis=1) - 1e-6).all()
    o.close()
    g.close()


# ---- 2. the records, bit for bit ------------------------------------------------------------------------------------------------------
UPLOAD_SHAPES = [(1, 1), (5, 3), (6, 5)]
_RECORD_CASES = [(s, "host", True) for s in SHAPES] + [(s, how, per) for s in UPLOAD_SHAPES
                                                        for how, per in (("host", False), ("device", True), ("device", False))]


def _upload(s, how, per, X, U, tracks, keep):
    """the path and every (index, track) through the host or the device entry points, per instance or shared (instance 3's)"""
    pick = (lambda a: a) if per else (lambda a: a[3])  # noqa: E731
    if how == "host":
        s.set_reference(pick(X), pick(U))
        for idx, t in tracks:
            s.set_constraint_track(idx, pick(t))
        return
    dx, du = DeviceArray(pick(X)), DeviceArray(pick(U))
    s.set_reference_device(dx.ptr, du.ptr, X.shape[1], per)
    keep += [dx, du]
    for idx, t in tracks:
        d = DeviceArray(pick(t))
        s.set_constraint_track_device(idx, d.ptr, t.shape[1], per)
        keep.append(d)


@pytest.mark.parametrize("shape,how,per", _RECORD_CASES,
                         ids=[f"{n}_{m}-{how}-{'per_instance' if per else 'shared'}" for (n, m), how, per in _RECORD_CASES])
def test_records_are_the_host_rows(A, hip_make, shape, how, per):
    """get_reference_terms() == _host_terms of the window and get_knot_params() == the track's rows, byte for byte, with the
    windows at rows 0, 7 and rows - 1 (the last row held on every knot); c on knot N uses Qf.  A second handle holds three knot
    constraints side by side -- the bound on [0, N), then CON_GOAL on knot N at offset 2 m of the record, an odd-width entry
    when n is odd, then a second CON_GOAL on [N - 2, N] at offset 2 m + n, an odd offset when n is odd.  get_knot_params reads a
    constraint's own knots only, so the zeros outside them cannot be read; the second goal shares knots N - 2 and N - 1 with
    the bound and knot N with the first goal instead, so an entry placed at a wrong offset of the record overwrites a
    neighbour that is read back -- and a tracking cost whose Q is NOT symmetric (q = -Q xref, include/altro_tracking.h: an index Q[j][i]
    in k_ref_terms gives other bits; no symmetric Q can tell the two apart, and no solve is made on this handle)."""
    n, m = shape
    kind = kind_of(A, n, m)
    Xref, Uref = KS.chain_path(n, m, B, ROWS)
    _, bound = KS.chain_bound(m, B, ROWS)
    src = (lambda a: a) if per else (lambda a: a[3:4])  # noqa: E731  (what the records must hold)
    keep = []
    s = KS.chain_tracking(A, hip_make, kind, n, m)
    _upload(s, how, per, Xref, Uref, [(s.knot_bound, bound)], keep)
    assert s.get_reference_offset() == 0  # a new path starts at its first row
    for offset in (0, 7, ROWS - 1):
        s.set_reference_offset(offset)
        s.set_track_offset(offset)
        Xw, Uw = KS.window(src(Xref), offset, np.arange(N + 1)), KS.window(src(Uref), offset, np.arange(N + 1))
        _same_terms(s.get_reference_terms(), _terms_of(n, m, Xw, Uw), f"{n}_{m} offset {offset}")
        _same_bytes(s.get_knot_params(s.knot_bound), KS.window(src(bound), offset, np.arange(N)), f"{n}_{m} offset {offset} bound")
    s.close()
    # three knot constraints in one record, a Q whose rows and columns differ
    Q, R, Qf = KS.chain_costs(n, m)
    Qns, Rns = Q + 0.25 * np.eye(n, k=1) - 0.125 * np.eye(n, k=-1), R + 0.25 * np.eye(m, k=1) - 0.125 * np.eye(m, k=-1)
    goal = np.cos(1.0 + Xref) + 0.01 * np.arange(n)
    goal2 = np.sin(2.0 + Xref) - 0.02 * np.arange(n)
    t = hip_make(n, m, N, B, A.F64)
    t.set_model(kind)
    t.set_uniform_step(KS.H)
    t.set_lqr_tracking_cost(0, N, Qns, Rns)
    t.set_lqr_tracking_cost(N, N + 1, Qf, R * 0)
    bi = t.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 2 * m)
    gi = t.add_knot_constraint(A.CON_GOAL, N, N + 1, n)
    gj = t.add_knot_constraint(A.CON_GOAL, N - 2, N + 1, n)
    t.set_initial_state(np.zeros(n))
    _upload(t, how, per, Xref, Uref, [(bi, bound), (gi, goal), (gj, goal2)], keep)
    for offset in (0, 7, ROWS - 1):
        t.set_reference_offset(offset)
        t.set_track_offset(offset)
        Xw, Uw = KS.window(src(Xref), offset, np.arange(N + 1)), KS.window(src(Uref), offset, np.arange(N + 1))
        _same_terms(t.get_reference_terms(), _terms_of(n, m, Xw, Uw, Q=Qns, R=Rns), f"{n}_{m} offset {offset}, Q not symmetric")
        _same_bytes(t.get_knot_params(bi), KS.window(src(bound), offset, np.arange(N)), f"{n}_{m} offset {offset} bound beside the goal")
        _same_bytes(t.get_knot_params(gi), KS.window(src(goal), offset, [N]), f"{n}_{m} offset {offset} goal")
        _same_bytes(t.get_knot_params(gj), KS.window(src(goal2), offset, [N - 2, N - 1, N]), f"{n}_{m} offset {offset} second goal")
    t.close()
    for d in keep:
        d.free()


# ---- 3. a constant path and constant tracks are an ordinary cost and ordinary constraints --------------------------------------------
def _constant_handle(A, make, n, m, dtype, knot_routed):
    """The chain pulled to xf = chain_goals (per instance) under the control bound +-0.6 and the goal constraint on knot N:
    as a tracking cost whose every path row is xf with two knot constraints of constant one-row tracks, or as set_lqr_cost with
    ordinary constraints, sent through the general kernels by a uniform set_steps."""
    batch = 5
    Q, R, Qf = KS.chain_costs(n, m)
    xf = chain_goals(n, m, N, batch)
    bound = np.array([-0.6] * m + [0.6] * m)
    s = make(n, m, N, batch, dtype)
    s.set_model(kind_of(A, n, m))
    s.set_uniform_step(KS.H)
    if knot_routed:
        s.set_lqr_tracking_cost(0, N, Q, R)
        s.set_lqr_tracking_cost(N, N + 1, Qf, R * 0)
        s.set_reference(xf[:, None, :])
        bi = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 2 * m)
        gi = s.add_knot_constraint(A.CON_GOAL, N, N + 1, n)
        s.set_constraint_track(bi, bound[None, :])
        s.set_constraint_track(gi, xf[:, None, :])
    else:
        s.set_lqr_cost(0, N, Q, R, xf, np.zeros(m))
        s.set_lqr_cost(N, N + 1, Qf, R * 0, xf, np.zeros(m))
        s.add_constraint(A.CON_CONTROL_BOUND, 0, N, bound)
        s.add_constraint(A.CON_GOAL, N, N + 1, xf)
        s.set_steps(np.full(N, KS.H, dtype=np.float32))
    s.set_initial_state(np.zeros(n))
    s.set_trajectory(None, np.zeros((N, m)))
    return s


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_constant_path_and_tracks_equal_ordinary_ones(A, hip_make, n, m, dtype_name):
    """tests/test_tracking_gpu.py::test_constant_path_equals_an_ordinary_cost and
    tests/test_knot_params_gpu.py::test_constant_track_equals_an_ordinary_constraint on every shape, fp64 and fp32 records:
    statistics, trajectory, gains, duals, penalties and initial state byte for byte."""
    dtype = getattr(A, dtype_name)
    t = _constant_handle(A, hip_make, n, m, dtype, True)
    u = _constant_handle(A, hip_make, n, m, dtype, False)
    t.solve()
    u.solve()
    a, b = _state(t), _state(u)
    assert a["stats"]["iterations_total"].min() > 1
    _same(a, b, f"{n}_{m} {dtype_name} constant path and tracks")
    t.close()
    u.close()


# ---- 4. step level against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_step_level_against_the_oracle(A, hip_make, n, m):
    """tests/test_tracking_gpu.py::test_step_level_against_the_oracle with its bars (those of tests/test_parity_gpu.py's
    step-level test), window at row 7."""
    o, g = _pair(A, hip_make, n, m, batch=5, offset=7)
    tag = f"{n}_{m} offset 7"
    for s in (o, g):
        s.rollout()
    _ledger.close(g.cost(), o.cost(), 1e-12, 0.0, f"{tag}: cost")
    for s in (o, g):
        s.update_expansions()
    for k in (0, 1, N // 2, N - 1, N):
        eo, eg = o.get_expansion(k), g.get_expansion(k)
        for key in ("lxx", "lx") + (("A", "B", "lxu", "luu", "lu") if k < N else ()):
            _ledger.close(eg[key], eo[key], 1e-10, 1e-12, f"{tag}: expansion {key}")
    _ledger.close(g.get_knot_costs(), o.get_knot_costs(), 1e-11, 1e-13, f"{tag}: knot costs")
    for s in (o, g):
        s.backward_pass()
        s.forward_pass()
    so, sg = o.get_stats(), g.get_stats()
    assert (so["alpha"] == sg["alpha"]).all() and (so["alpha"] > 0).all()
    _ledger.close(sg["cost"], so["cost"], 1e-9, 0.0, f"{tag}: cost after the forward pass")
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    _ledger.close(Xg, Xo, 1e-8, 1e-10, f"{tag}: X after the forward pass")
    _ledger.close(Ug, Uo, 1e-8, 1e-10, f"{tag}: U after the forward pass")
    o.close()
    g.close()


# ---- 5. fp32 records ---------------------------------------------------------------------------------------------------------------------
# Bars of chain_tracking(dtype=A.F32) against the record-rounding oracle (dtype 2, per knot), batch 40, window at row 7
# (X, U abs; K norm-wise).  Baseline: what tests/test_model_shapes_gpu.py::test_fp32_records measures for the same shape at batch
# 40 on the MI355X (its ledger lines, second row of each entry); the bar is that file's bar over its measurement (_F32_BARS:
# 10 - 20 x, rounded up to 1 / 2 / 5, never below 1e-14 abs / 1e-13 norm-wise).
# This problem itself measures two to four orders below its baseline on the MI355X (third column; 6 to 14 iterations where
# chain_al takes 10 to 20 and more): (13,2) uses 3e-4 of its X bar, (5,3) 4e-2, and K agrees to the last bit on all five.
#   shape     baseline X, U, K                 bar X, U, K              this problem measures X, U, K
_F32_TRACK_BARS = {
    (1, 1): ((2.2e-16, 3.6e-15, 0.0), (1e-14, 5e-14, 1e-13), (1.1e-16, 8.9e-16, 0.0)),
    (2, 2): ((3.1e-15, 5.7e-14, 0.0), (5e-14, 1e-12, 1e-13), (1.1e-16, 1.8e-15, 0.0)),
    (3, 5): ((4.8e-13, 7.3e-12, 1.9e-10), (5e-12, 1e-10, 2e-09), (0.0, 0.0, 0.0)),
    (5, 3): ((1.6e-09, 5.2e-08, 1.3e-09), (2e-08, 1e-06, 2e-08), (8.4e-10, 1.3e-08, 0.0)),
    (13, 2): ((4.1e-08, 2.7e-07, 1.1e-07), (5e-07, 5e-06, 2e-06), (1.4e-10, 2.5e-10, 0.0)),
}
assert all(_F32_TRACK_BARS[s][1] == _F32_BARS[(s, 40)] for s in F32_SHAPES)


@pytest.mark.parametrize("n,m", F32_SHAPES, ids=ids(F32_SHAPES))
def test_fp32_records(A, hip_make, n, m):
    """ALTRO_F32 records under a tracking cost and a knot constraint (the reference-term and knot-parameter records stay
    fp64; the expansion and gain records they feed are fp32) against the record-rounding oracle, as
    tests/test_model_shapes_gpu.py::test_fp32_records: status and both iteration counts exact."""
    kind = kind_of(A, n, m)
    o = KS.chain_tracking(A, oracle_of(A, n, m), kind, n, m, batch=40, offset=7, dtype=2, per_knot=True)
    g = KS.chain_tracking(A, hip_make, kind, n, m, batch=40, offset=7, dtype=A.F32)
    o.solve()
    g.solve()
    so, sg = o.get_stats(), g.get_stats()
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (f, np.flatnonzero(so[f] != sg[f])[:8])
    assert (so["status"] == A.SOLVED).all()
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    tag = f"{n}_{m} offset 7 fp32 records"
    bX, bU, bK = _F32_TRACK_BARS[(n, m)][1]
    _all([lambda: _ledger.close(Xg, Xo, 0.0, bX, f"{tag}: X"),
          lambda: _ledger.close(Ug, Uo, 0.0, bU, f"{tag}: U"),
          lambda: _ledger.close_normwise(g.get_gains()[0], o.get_gains()[0], bK, f"{tag}: K, normwise")])
    o.close()
    g.close()


# ... and of problems.tracking_slalom(dtype=A.F32), the built-in unicycle, batch 40, in the same way (X, U abs; K norm-wise; the
# final cost relative): what the MI355X measures against the record-rounding oracle, times MARGIN, rounded up to 1 / 2 / 5,
# never below _F32_BARS's floors of 1e-14 abs / 1e-13 norm-wise.  No earlier test solves a tracking cost with fp32 records, so
# the baseline is this problem's own ledger line; the bars tests/test_f32_gpu.py holds for the unicycle's goal problem (X 1e-6,
# U 1e-5, K 1e-4, cost 1e-7) lie nine orders above it.
#   offset   measured X, U, K, cost              bar X, U, K, cost
_F32_SLALOM_BARS = {
    0: ((4.4e-16, 1.9e-15, 0.0, 3.8e-14), (1e-14, 2e-14, 1e-13, 5e-13)),
    12: ((6.1e-16, 4.4e-15, 0.0, 3.4e-14), (1e-14, 5e-14, 1e-13, 5e-13)),
}
assert all(bar == tuple(max(_bar(x), floor) if x else floor for x, floor in zip(got, (1e-14, 1e-14, 1e-13, 1e-14)))
           for got, bar in _F32_SLALOM_BARS.values())


@pytest.mark.parametrize("offset", [0, 12])
def test_fp32_records_tracking_slalom(A, P, oracle_make, hip_make, offset):
    """The built-in unicycle: problems.tracking_slalom(dtype=A.F32) against the record-rounding oracle given one cost per knot:
    status and both iteration counts exact, X, U, K and the final cost within _F32_SLALOM_BARS."""
    o = P.tracking_slalom(oracle_make, batch=40, N=24, rows=37, offset=offset, dtype=2, per_knot=True)
    g = P.tracking_slalom(hip_make, batch=40, N=24, rows=37, offset=offset, dtype=A.F32)
    o.solve()
    g.solve()
    so, sg = o.get_stats(), g.get_stats()
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (f, np.flatnonzero(so[f] != sg[f])[:8])
    assert (so["status"] == A.SOLVED).all()
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    tag = f"slalom 3_2 offset {offset} fp32 records"
    bX, bU, bK, bJ = _F32_SLALOM_BARS[offset][1]
    _all([lambda: _ledger.close(Xg, Xo, 0.0, bX, f"{tag}: X"),
          lambda: _ledger.close(Ug, Uo, 0.0, bU, f"{tag}: U"),
          lambda: _ledger.close_normwise(g.get_gains()[0], o.get_gains()[0], bK, f"{tag}: K, normwise"),
          lambda: _ledger.close(sg["cost"], so["cost"], bJ, 0.0, f"{tag}: stat cost")])
    o.close()
    g.close()


# ---- 6. gain-chunk boundaries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,horizon", [((1, 1), 127), ((5, 3), 33)], ids=["1_1-N127", "5_3-N33"])
def test_gain_chunk_horizons(A, hip_make, shape, horizon):
    """One knot past kBwdChunk = 126 (4 x 4 kernel) and kM16Chunk = 32 (16 x 16 kernel): the backward kernels are those of the
    ordinary path, fed by k_expansions_trk here.  Batch 8, offset 0, a path of N + 1 rows, the bars of the whole solves.  Both
    solve on the oracle: (5,3) at N = 33 in 8 to 14 iterations, 2 to 5 outer (X and the violation TIGHT, U and the cost by its
    own entry of _SOLVE_BARS, measured at this horizon); (1,1) at N = 127 in 20 to 24, 6 or 7 outer (TIGHT).
    The ramp of the bound closes at row 100 and the library refuses a track whose lower bound is not below its upper one, so
    the track of N = 127 ends at row 99, which the window holds (_knot_shapes_common.BOUND_ROWS)."""
    n, m = shape
    o, g = _pair(A, hip_make, n, m, batch=8, N=horizon, rows=horizon + 1)
    tag = f"{n}_{m} N {horizon} offset 0"
    so, _ = _against_the_oracle(A, o, g, tag, _bars(shape, 0, horizon))
    assert (so["status"] == A.SOLVED).all()
    (Ko, do), (Kg, dg) = o.get_gains(), g.get_gains()
    assert np.abs(Ko[:, -1]).max() > 0 and np.abs(Ko[:, 0]).max() > 0  # gains on both sides of the chunk boundary
    # K: the bar tests/test_knot_params_gpu.py::test_ramped_bounds_against_the_oracle holds for the gains of a whole solve
    _ledger.close_normwise(Kg, Ko, 1e-6, f"{tag}: K, normwise")
    o.close()
    g.close()


# ---- 7. the window and the advance ----------------------------------------------------------------------------------------------------
WINDOW_SHAPES = [(1, 2), (7, 3), (13, 2)]


def _records(s):
    return s.get_reference_terms() + (s.get_knot_params(s.knot_bound),)


def _same_records(a, b, what):
    for name, x, y in zip(("q", "r", "c", "bound"), a, b):
        assert x.tobytes() == y.tobytes(), (what, name)


@pytest.mark.parametrize("n,m", WINDOW_SHAPES, ids=ids(WINDOW_SHAPES))
def test_window_equals_a_fresh_handle(A, hip_make, n, m):
    """A handle solved at row 0 and then moved to row 7 (both offsets, a new initial state, the zero guess) against a fresh
    handle built at row 7 and a fresh handle given rows 7 .. 7 + N on the host: terms, knot parameters and the solve, byte
    for byte."""
    kind = kind_of(A, n, m)
    Xref, Uref = KS.chain_path(n, m, B, ROWS)
    _, bound = KS.chain_bound(m, B, ROWS)
    moved = KS.chain_tracking(A, hip_make, kind, n, m)
    moved.solve()
    fresh = KS.chain_tracking(A, hip_make, kind, n, m, offset=7)
    rows = KS.chain_tracking(A, hip_make, kind, n, m, offset=7)
    rows.set_reference(KS.window(Xref, 7, np.arange(N + 1)), KS.window(Uref, 7, np.arange(N + 1)))
    rows.set_constraint_track(rows.knot_bound, KS.window(bound, 7, np.arange(N)))
    rows.set_track_offset(0)
    moved.set_reference_offset(7)
    moved.set_track_offset(7)
    moved.set_initial_state(fresh.get_initial_state())
    moved.set_trajectory(None, np.zeros((N, m)))
    assert (moved.get_reference_offset(), moved.get_track_offset()) == (7, 7)
    assert (rows.get_reference_offset(), rows.get_track_offset()) == (0, 0)
    for other, what in ((moved, "moved"), (rows, "host rows")):
        _same_records(_records(other), _records(fresh), f"{n}_{m} {what}")
    for s in (moved, fresh, rows):
        s.solve()
    want = _state(fresh)
    assert want["stats"]["iterations_total"].min() > 1
    _same(_state(moved), want, f"{n}_{m} moved")
    _same(_state(rows), want, f"{n}_{m} host rows")
    for s in (moved, fresh, rows):
        s.close()


@pytest.mark.parametrize("n,m", WINDOW_SHAPES, ids=ids(WINDOW_SHAPES))
def test_advance_and_mpc_run(A, hip_make, n, m):
    """mpc_advance(3) on a solved handle: both offsets read 3 and both records are the host rows of the windows at row 3.
    mpc_run (3 cycles of shift 2, the disturbance of _mpc_common.disturbance) against the caller's own loop of solve and
    advance: the logs and everything left on the handle, bit for bit
    (tests/test_tracking_gpu.py::test_mpc_loops_equal_the_callers_loop)."""
    kind = kind_of(A, n, m)
    Xref, Uref = KS.chain_path(n, m, B, ROWS)
    _, bound = KS.chain_bound(m, B, ROWS)
    s = KS.chain_tracking(A, hip_make, kind, n, m)
    s.solve()
    X = s.get_trajectory()[0]
    s.mpc_advance(3)
    assert (s.get_reference_offset(), s.get_track_offset()) == (3, 3)
    _same_terms(s.get_reference_terms(), _terms_of(n, m, KS.window(Xref, 3, np.arange(N + 1)), KS.window(Uref, 3, np.arange(N + 1))),
                f"{n}_{m} advanced to row 3")
    _same_bytes(s.get_knot_params(s.knot_bound), KS.window(bound, 3, np.arange(N)), f"{n}_{m} advanced to row 3, bound")
    _same_bytes(s.get_initial_state(), X[:, 3], f"{n}_{m} advanced x0")
    s.close()
    cycles, shift = 3, 2
    W = M.disturbance(cycles, B, n)
    a = KS.chain_tracking(A, hip_make, kind, n, m)
    b = KS.chain_tracking(A, hip_make, kind, n, m)
    Xl, Ul, it, st = [], [], [], []
    for c in range(cycles):
        a.solve()
        X, U = a.get_trajectory()
        Xl.append(a.get_initial_state()[:, None])
        Xl.append(X[:, 1:shift])
        Ul.append(U[:, :shift])
        it.append(a.get_stats()["iterations_total"])
        st.append(a.get_stats()["status"])
        a.mpc_advance(shift, w=W[c])
    Xl.append(a.get_initial_state()[:, None])
    out = b.mpc_run(cycles, shift, W)
    assert out["X_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Xl, axis=1)).tobytes()
    assert out["U_cl"].tobytes() == np.ascontiguousarray(np.concatenate(Ul, axis=1)).tobytes()
    assert np.array_equal(out["iterations"], np.stack(it, axis=1)) and np.array_equal(out["status"], np.stack(st, axis=1))
    assert np.stack(it, axis=1).min() > 0
    for h in (a, b):
        assert (h.get_reference_offset(), h.get_track_offset()) == (cycles * shift, cycles * shift)
    _same(_state(a), _state(b), f"{n}_{m} mpc_run")
    _same_records(_records(a), _records(b), f"{n}_{m} mpc_run")
    _same_bytes(a.get_knot_params(a.knot_bound), KS.window(bound, cycles * shift, np.arange(N)), f"{n}_{m} mpc_run bound")
    a.close()
    b.close()


# ---- 8. closed-loop tracking ----------------------------------------------------------------------------------------------------------
TRACK_SHAPES = [(2, 2), (9, 1), (3, 5)]


@pytest.mark.parametrize("n,m", TRACK_SHAPES, ids=ids(TRACK_SHAPES))
def test_mpc_track(A, hip_make, n, m):
    """k_mpc_track_trk on a solved handle, window at row 7, batch 5.  One sample, no disturbance: the plan's rollout bits (the
    kernel's comment promises them), and `cost` is the tracking cost over the window's rows evaluated in np.longdouble, to 1e-12
    relative (the bar of tests/test_tracking_gpu.py::test_mpc_track_cost_is_the_tracking_cost).  Four samples of a seeded
    dx0: states, controls and the largest deviations against the closed loop rolled out in numpy from the downloaded gains,
    to the trajectory bar (1e-7 relative + 1e-9 absolute, tests/test_mpc_track_gpu.py); the violation against the ramped
    bound of each knot in numpy to the same bar, and exactly against altro_max_violation of a second handle
    (tests/test_mpc_track_gpu.py::test_statistics_against_existing_entry_points)."""
    batch, offset, S = 5, 7, 4
    kind = kind_of(A, n, m)
    s = KS.chain_tracking(A, hip_make, kind, n, m, batch=batch, offset=offset)
    s.solve()
    s.rollout()
    Xbar, Ubar = s.get_trajectory()
    K, _ = s.get_gains()
    tag = f"{n}_{m} offset {offset}"
    one = s.mpc_track(N, 1)
    assert one["X_cl"][:, 0].tobytes() == Xbar.tobytes() and one["U_cl"][:, 0].tobytes() == Ubar.tobytes()
    assert (one["stats"]["steps_done"] == N).all() and (one["stats"]["max_dx"] == 0).all() and (one["stats"]["max_du"] == 0).all()
    Q, R, Qf = KS.chain_costs(n, m)
    Xref, Uref = KS.chain_path(n, m, batch, ROWS)
    Xw, Uw = KS.window(Xref, offset, np.arange(N + 1)), KS.window(Uref, offset, np.arange(N + 1))
    J = np.array([float(KS.tracking_cost(Q, R, Qf, Xw[b], Uw[b], Xbar[b], Ubar[b])) for b in range(batch)])
    _ledger.close(one["stats"]["cost"][:, 0], J, 1e-12, 0.0, f"{tag}: mpc_track cost against the tracking cost on the host")
    # four samples under the feedback policy
    bb, jj, ii = np.meshgrid(np.arange(batch), np.arange(S), np.arange(n), indexing="ij")
    dx0 = 1e-2 * np.sin(1.0 + 3.0 * jj + 5.0 * bb + 7.0 * ii)
    out = s.mpc_track(N, S, dx0=dx0)
    st = out["stats"]
    assert (st["steps_done"] == N).all()
    x = (s.get_initial_state()[:, None, :] + dx0).reshape(batch * S, n)
    Xr, Ur = [x], []
    for k in range(N):
        dx = x.reshape(batch, S, n) - Xbar[:, None, k]
        u = (Ubar[:, None, k] + np.einsum("bil,bsl->bsi", K[:, k], dx)).reshape(batch * S, m)
        x = chain_rk4(x, u[:, None, :], float(KS.H), n, m)
        Ur.append(u)
        Xr.append(x)
    Xr, Ur = np.stack(Xr, axis=1).reshape(batch, S, N + 1, n), np.stack(Ur, axis=1).reshape(batch, S, N, m)
    _ledger.close(out["X_cl"], Xr, RTOL, ATOL, f"{tag}: closed-loop X")
    _ledger.close(out["U_cl"], Ur, RTOL, ATOL, f"{tag}: closed-loop U")
    _ledger.close(st["max_dx"], np.abs(Xr - Xbar[:, None]).max(axis=(2, 3)), RTOL, ATOL, f"{tag}: max_dx")
    _ledger.close(st["max_du"], np.abs(Ur - Ubar[:, None]).max(axis=(2, 3)), RTOL, ATOL, f"{tag}: max_du")
    ub = KS.window(KS.chain_bound(m, batch, ROWS)[0][:, :, None], offset, np.arange(N))  # [B][N][1]
    viol = np.maximum(np.abs(Ur) - ub[:, None], 0.0).max(axis=(2, 3))
    assert (viol > 0).any()  # the feedback pushes a saturated control past the ramped bound
    _ledger.close(st["violation"], viol, RTOL, ATOL, f"{tag}: closed-loop violation")
    for smp in range(S):  # (one handle per sample: the instance decides path and track)
        con = KS.chain_tracking(A, hip_make, kind, n, m, batch=batch, offset=offset)
        con.set_trajectory(out["X_cl"][:, smp], out["U_cl"][:, smp])
        assert st["violation"][:, smp].tobytes() == con.max_violation().tobytes(), smp
        con.close()
    s.close()


# ---- 9. multi-start on a knot-routed handle --------------------------------------------------------------------------------------------
PROBLEMS, STARTS, N_MS, ROWS_MS = 6, 4, 24, 24 + 13
COST_BAR = 1e-10  # relative: the bar of the final cost against the oracle (tests/test_knot_params_gpu.py)
COLUMN = ("X", "U", "K", "d", "lam", "rho", "cval", "costs")  # what a spread copies (tests/test_multistart_gpu.py)


def _snapshot(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    q, r, c = s.get_reference_terms()
    return dict(X=X.copy(), U=U.copy(), K=K.copy(), d=d.copy(), lam=s.get_duals(), rho=s.get_penalties(), cval=s.get_constraint_values(),
                costs=s.get_knot_costs(), x0=s.get_initial_state(), stats=s.get_stats().copy(), q=q, r=r, c=c,
                circle=s.get_knot_params(s.knot_circle), bound=s.get_knot_params(s.knot_bound))


RECORDS = ("q", "r", "c", "circle", "bound")


def _margins(stats):
    """relative distance between the winner's cost and the runner-up's, per problem (every start solved)"""
    c = np.sort(stats["cost"].reshape(PROBLEMS, STARTS), axis=1)
    return (c[:, 1] - c[:, 0]) / np.abs(c[:, 0])


@pytest.fixture(scope="module")
def oracle_starts(A, P, oracle_make):
    o = KS.moving_obstacles_starts(A, P, oracle_make, PROBLEMS, STARTS, N_MS, ROWS_MS, per_knot=True)
    o.solve()
    st = o.get_stats().copy()
    o.close()
    return st


def test_multistart_problem_is_moving_obstacles(A, P, oracle_make):
    """_knot_shapes_common.moving_obstacles_starts states problems.moving_obstacles again, laid out as problems x starts (the
    library's builder takes one parameter set per instance).  So that the two cannot drift apart: with one start per problem
    and that problem's own guess U = (0.1, 0.1), every call arrives as from problems.moving_obstacles -- the oracle's answer
    is the same to the byte (CPU work: no kernel runs here)."""
    for offset in (0, 6):
        a = KS.moving_obstacles_starts(A, P, oracle_make, PROBLEMS, 1, N_MS, ROWS_MS, offset=offset, per_knot=True, ladder=[[0.1, 0.1]])
        b = P.moving_obstacles(oracle_make, batch=PROBLEMS, N=N_MS, rows=ROWS_MS, offset=offset, per_knot=True)
        for s in (a, b):
            s.solve()
        assert a.get_stats().tobytes() == b.get_stats().tobytes()
        for x, y in zip(a.get_trajectory() + a.get_gains(), b.get_trajectory() + b.get_gains()):
            assert x.tobytes() == y.tobytes()
        a.close()
        b.close()


def test_multistart_oracle_inputs_exercise_the_rule(A, oracle_starts):
    """On the oracle's statistics alone: every start solves, a problem exists whose start 0 is not the winner, and at most one
    problem of six has its winner and runner-up closer than the cost bar (such a problem is left out of the comparison of
    winners).  Measured on the CPU with _knot_shapes_common.LADDER: winners 1, 3, 2, 0, 3, 1, narrowest margin 4.1e-10.
    problems.slalom_path and moving_obstacle_tracks repeat their parameters with b mod 5: problem 5 is problem 0 again, bit
    for bit, so five of the six problems are distinct and the sixth can add no winner of its own."""
    assert (oracle_starts["status"] == A.SOLVED).all()
    win = MS.rule_winners(oracle_starts, STARTS)
    assert (win != 0).any() and len(set(win.tolist())) > 1
    close = np.flatnonzero(_margins(oracle_starts) <= COST_BAR)
    _ledger.count("multi-start: problems whose oracle margin is within the cost bar", len(close), 1, close)
    assert len(close) <= 1


def test_multistart_select(A, P, hip_make, oracle_starts):
    """multistart_select == the host rule on the GPU's own statistics, index for index; == the host rule on the oracle's
    statistics wherever the oracle's margin exceeds the cost bar.  The solve itself: schedules exact, cost to the cost bar."""
    s = KS.moving_obstacles_starts(A, P, hip_make, PROBLEMS, STARTS, N_MS, ROWS_MS)
    s.solve()
    sg, so = s.get_stats(), oracle_starts
    for f in ("status", "iterations_total", "iterations_outer"):
        assert np.array_equal(sg[f], so[f]), (f, sg[f].reshape(PROBLEMS, STARTS), so[f].reshape(PROBLEMS, STARTS))
    _ledger.close(sg["cost"], so["cost"], COST_BAR, 0.0, "multi-start 3_2 offset 0: stat cost")
    before = _snapshot(s)
    win = s.multistart_select(STARTS)
    assert np.array_equal(win, MS.rule_winners(sg, STARTS)), (win, MS.rule_winners(sg, STARTS))
    clear = _margins(so) > COST_BAR
    _ledger.count("multi-start: problems left out of the comparison of winners", (~clear).sum(), 1, np.flatnonzero(~clear))
    assert (~clear).sum() <= 1
    assert np.array_equal(win[clear], MS.rule_winners(so, STARTS)[clear]), (win, MS.rule_winners(so, STARTS))
    after = _snapshot(s)
    for name in COLUMN + RECORDS + ("x0",):  # select changes nothing on the handle
        assert after[name].tobytes() == before[name].tobytes(), name
    s.close()


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_multistart_spread(A, P, hip_make, dtype_name):
    """multistart_spread leaves every start's X, U, gains, duals, penalties, constraint values and knot costs byte-equal to
    the winner's column, and the reference terms and knot parameters -- identical within a problem, never copied -- untouched."""
    s = KS.moving_obstacles_starts(A, P, hip_make, PROBLEMS, STARTS, N_MS, ROWS_MS, dtype=getattr(A, dtype_name))
    s.solve()
    before = _snapshot(s)
    want = MS.rule_winners(before["stats"], STARTS)
    win = s.multistart_spread(STARTS)
    assert np.array_equal(win, want)
    if dtype_name == "F64":  # (the winners of the oracle: a spread that always copied start 0 would not pass)
        assert len(set(win.tolist())) > 1
    src = np.repeat(np.arange(PROBLEMS) * STARTS + win, STARTS)
    after = _snapshot(s)
    for name in COLUMN:
        assert after[name].tobytes() == np.ascontiguousarray(before[name][src]).tobytes(), name
    for name in RECORDS + ("x0",):
        assert after[name].tobytes() == before[name].tobytes(), name
    assert after["lam"].shape[1] > 0 and after["stats"].tobytes() == before["stats"].tobytes()
    s.close()


@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
def test_mpc_run_multistart_is_the_callers_loop(A, P, hip_make, dtype_name):
    """mpc_run_multistart(starts = 4, cycles = 3, shift = 2, dU) against the caller's loop of solve, spread, advance and
    perturb: the logs, everything left on the handle and both windows -- which read row 6 at the end -- bit for bit."""
    cycles, shift = 3, 2
    a = KS.moving_obstacles_starts(A, P, hip_make, PROBLEMS, STARTS, N_MS, ROWS_MS, dtype=getattr(A, dtype_name))
    b = KS.moving_obstacles_starts(A, P, hip_make, PROBLEMS, STARTS, N_MS, ROWS_MS, dtype=getattr(A, dtype_name))
    g = np.arange(STARTS, dtype=np.float64)
    dU = np.broadcast_to(np.stack([0.02 * g, -0.03 * g], axis=1)[:, None, :], (STARTS, N_MS, 2)).copy()
    rec = []
    for c in range(cycles):
        a.solve()
        st = a.get_stats()
        win = a.multistart_spread(STARTS)
        X, U = a.get_trajectory()
        rec.append(dict(it=st["iterations_total"].copy(), status=st["status"].copy(), win=win, X=X.copy(), U=U.copy(), x0=a.get_initial_state()))
        a.mpc_advance(shift)
        a.multistart_perturb(STARTS, dU)
    out = b.mpc_run_multistart(STARTS, cycles, shift, dU=dU)
    for h in (a, b):
        assert (h.get_reference_offset(), h.get_track_offset()) == (cycles * shift, cycles * shift) == (6, 6)
    fa, fb = _snapshot(a), _snapshot(b)
    for name in COLUMN + RECORDS + ("x0",):
        assert fa[name].tobytes() == fb[name].tobytes(), name
    assert fa["stats"].tobytes() == fb["stats"].tobytes()
    for c in range(cycles):
        assert np.array_equal(out["iterations"][:, c], rec[c]["it"]) and np.array_equal(out["status"][:, c], rec[c]["status"])
        assert np.array_equal(out["winner"][:, c], rec[c]["win"]), c
        rows = slice(c * shift, (c + 1) * shift)
        assert out["X_cl"][:, rows].tobytes() == np.ascontiguousarray(rec[c]["X"][:, :shift]).tobytes()
        assert out["U_cl"][:, rows].tobytes() == np.ascontiguousarray(rec[c]["U"][:, :shift]).tobytes()
        assert out["X_cl"][:, c * shift].tobytes() == rec[c]["x0"].tobytes()
    assert np.stack([r["it"] for r in rec]).min() > 0
    # the windows at row 6 hold the host rows
    circles, bounds = P.moving_obstacle_tracks(PROBLEMS, N_MS, ROWS_MS)
    _same_bytes(fb["circle"], np.repeat(KS.window(circles, 6, np.arange(1, N_MS)), STARTS, axis=0), "circle track at row 6")
    _same_bytes(fb["bound"], np.repeat(KS.window(bounds, 6, np.arange(N_MS)), STARTS, axis=0), "bound track at row 6")
    a.close()
    b.close()
