"""The termination paths and the solver options on a knot-routed handle (Engine::KnotRouted: a tracking cost or a knot
constraint), against the oracle.

Such a handle never runs k_forward2, k_sweep_fused, k_sweep_loop or the segments: every solve goes through the *_trk twins
(k_expansions_trk, k_forward_trk, k_knot_costs_trk, k_mpc_track_trk), the general kernel bodies over CtxGK.
tests/test_termination_gpu.py and tests/test_options_gpu.py build their scenarios from ordinary costs and constraints and never
reach a twin; the tests of the knot-routed features run default options on solves that succeed.  Here the device handle has the
tracking cost (set_lqr_tracking_cost + set_reference) and the knot constraints (add_knot_constraint + set_constraint_track) at a
non-zero window offset; the oracle is given the same rows as one ordinary set_lqr_cost / add_constraint per knot.  Path and
tracks differ from knot to knot and from instance to instance (tests/_knot_term_common.py): a kernel that reads row k +- 1, or
another instance's row, changes the schedule.

Two problems: MO = problems.moving_obstacles(batch 10, N 24, 37 rows, offset 5), five parameter sets b mod 5; GU = the
give-up problem of test_termination_gpu.py per knot (_knot_term_common.gu).  Every scenario has a test without a GPU
(..._on_the_oracle: the oracle alone reaches the path, so the GPU test beside it cannot pass vacuously) and a GPU test against
the oracle; the oracle's results are computed once and shared, read only.

  1  give-up, step level: GU on the unicycle at N = 40 and N = 160 (the written knots cross kBwdChunk = 126) and on the (5,3)
     chain (k_backward_mfma16's chunk of 32); one case with fp32 records against the record-rounding oracle
  2  give-up, whole solves: default trials and no trial at all (the only way status 9 survives a solve), batch 9; batch 2050 on
     four chains
  3  MO under every option set of MO_SETS: ALTRO_MAX_PENALTY, the rollout limits (all instances, and a mix of limit and
     solved), the iteration caps, line searches of 0, 3 and 40 trials; the 3-trial set and maximum_penalty = 1000 again at
     batch 2050 on four chains (finished instances beside long runners: the compaction lists of the sweeps)
  4  the rollout limits at step level: the first failing step is the control of knot 0 (with states over their limit later),
     or the state of knot N alone; the check switched off
  5  per-knot steps: MO whole solve and one sweep, GU with no trial
  6  the history rows of MO, default and 3 trials
  7  the cost-to-go: replayed after a whole solve against recorded during it, bit for bit, and against the oracle's; after the
     window moved the records are refused
  8  warm start: solve, reset_duals = 0, initial_penalty = 0, mpc_advance(3), solve

Statuses, iteration counts, alpha, the regularisation and max_penalty are compared with ==; values go through the ledger
(tests/_ledger.py) to the project's bars: whole solves on knot problems X, U 1e-7 relative + 1e-9
(test_knot_params_gpu.py::_compare_with_oracle), the duals 1e-7 relative + 1e-9 x the instance's largest penalty (the form of
test_parity_gpu.py's dual bar: an error e in a constraint value is rho e in lambda - rho c), the penalties 1e-7 relative; step
level 1e-9 relative + 1e-11, K 1e-9 norm-wise (test_model_shapes_gpu.py::test_gain_chunk_horizons); the history the bars of
test_parity_gpu.py::test_history_matches_oracle (violations as the gradient there).

Reached on the MI355X: final statuses 0, 2, 3, 5, 6, 7, 8 and 9, status_ilqr 1, 2, 3 and 9 at step level.

Found: nothing to fix.  Every scenario passed as the kernels stood, every toleranced comparison below 2 % of its bar
(profiles/r06_parity_errors.json; the largest: the gradient history of the 3-trial set, 4e-9 relative), so no bar was widened.
The 40-trial set never met the stale-c_ fallback of DESIGN section 7 (a later round of 20 without a successful rollout): its
schedule is the oracle's.  One expectation of mine was wrong and the test now states the code's: a handle that holds
cost-to-go records keeps answering with them after the window moved (they are the last backward pass's); only a handle
without records is refused (test_ctg).

No test: kCostIncrease (4), unreachable (see test_termination_gpu.py).  The large batches are compared with the oracle's
instance of the same parameter set and, bit for bit, with the device's batch of 10, not with an oracle run of 2050.  The
oracle got altro_set_penalties' counterpart (oracle_set_penalties) for the warm start.

Three mutants, argued from the code (none was run):
  - CtxGK::par reading knot k + 1 for kParPerKnotCon: every knot constraint takes the next row of its track.  GU's middle
    third starts outside the bound, so the first expansions already hold rho (u - ub_k): the row of knot k + 1 is 0.001
    wider and d moves by ~1e-3 of itself -- test_giveup_step (d to 1e-9), on every case; at knot N - 1 the read leaves the
    constraint's knots.  On MO the bound and both circles move with the row: test_mo_options[default] loses the schedule.
  - forward_kernel's last_status initialised to kUnsolved when ls_max == 0: the status the backward pass left is lost, the
    instances that gave up iterate on to kMaxInnerIterations instead of ending with 9 after one iteration --
    test_giveup_solve[*-ls0] (status, iterations_total; the five cases, per-knot steps included).  test_mo_options[ls0] does
    not see it: no backward pass fails there.
  - k_expansions_trk launched without the order list in a chain (Engine::EnqueueSweep's dense launch, all = 2: models with
    n m < 12, the unicycle here, from the second sweep on while a quarter of the chain still iterates): the kernel rebuilds
    the chain's list through order_list / order_count, so the launch writes through a null pointer -- every whole solve of
    the unicycle here has such a sweep, the first is test_giveup_solve[unicycle_3_2-N40-default]; on four chains
    test_mo_options_on_four_chains and
    test_giveup_solve[unicycle_3_2-N40-chains].  A mutant that merely skipped the rebuild would leave the list of the sweep
    before, the same instances in another order: same results, by construction nothing a parity test can see."""
import numpy as np
import pytest

import _knot_term_common as C
import _ledger
import _mpc_common as M
from test_model_shapes_gpu import kind_of, oracle_of
from test_termination_gpu import SOLVE_FIELDS, _al_result, _exact, _once, _result, _threads

N = C.N_MO
RTOL, ATOL = 1e-7, 1e-9          # whole solves on knot problems
STEP_RTOL, STEP_ATOL = 1e-9, 1e-11  # step level; K 1e-9 norm-wise
MO_FIELDS = SOLVE_FIELDS + ("alpha", "max_penalty")
MOVING_CONS = [(1, N, 2, False), (0, N, 4, False)]  # problems.moving_obstacles: (k_begin, k_end, rows, equality)
BIG = 2050  # four chains; no multiple of 64, of 5 or of 3
CHAINS = {"ALTRO_HIP_CHAINS": "4"}


def _cmp_solve(tag, g, o, duals=True):
    _ledger.close(g["X"], o["X"], RTOL, ATOL, f"{tag}: X")
    _ledger.close(g["U"], o["U"], RTOL, ATOL, f"{tag}: U")
    if duals:
        scale = np.maximum(o["pen"].max(axis=1, keepdims=True), 1.0)
        _ledger.close(g["lam"] / scale, o["lam"] / scale, RTOL, ATOL, f"{tag}: duals over the instance's largest penalty")
        _ledger.close(g["pen"], o["pen"], RTOL, 0.0, f"{tag}: penalties")


def _cmp_step(tag, g, o, gains=True):
    _ledger.close(g["X"], o["X"], STEP_RTOL, STEP_ATOL, f"{tag}: X")
    _ledger.close(g["U"], o["U"], STEP_RTOL, STEP_ATOL, f"{tag}: U")
    if gains:
        _ledger.close_normwise(g["K"], o["K"], 1e-9, f"{tag}: K")
        _ledger.close(g["d"], o["d"], STEP_RTOL, STEP_ATOL, f"{tag}: d")


def _knot_routed(g):
    """the solve ran on the batched sweeps alone: no persistent kernel, no device loop, no twin, no segment column"""
    tm = g.get_timing()
    assert (tm["fused_sweeps"], tm["loop_iterations"], tm["twin_workgroups"], tm["segment_columns"]) == (0, 0, 0, 0) and tm["sweeps"] >= 1, tm


def _sets(a):
    """[5]: the value of every parameter set, which the instances b and b + 5 share"""
    a = np.asarray(a)
    assert np.array_equal(a.reshape(-1, 5), np.tile(a[:5], (len(a) // 5, 1))), a
    return a[:5]


# ---- 1. give-up, step level ---------------------------------------------------------------------------------------------------
# (model, (n, m), N, ks)
GU_CASES = [("unicycle", (3, 2), 40, 6), ("unicycle", (3, 2), 160, 20), ("chain", (5, 3), 40, 4)]
GU_IDS = [f"{mo}_{n}_{m}-N{N_}" for mo, (n, m), N_, _ in GU_CASES]
GU_STEP = [(c, "f64") for c in GU_CASES] + [(GU_CASES[0], "f32")]
GU_STEP_IDS = [f"{mo}_{n}_{m}-N{N_}-{r}" for (mo, (n, m), N_, _), r in GU_STEP]


def _gu(A, make, case, device, batch=9, dtype=0, **kw):
    """GU of ``case``: ``device`` -- the knot-routed statement for the library, else the per-knot one for the oracle"""
    model, (n, m), N_, ks = case
    if model == "unicycle":
        kind = A.MODEL_UNICYCLE
    else:
        kind = kind_of(A, n, m) if device else A.MODEL_USER_BASE
    return C.gu(A, make, kind, n, m, N_, ks, batch, not device, dtype=dtype, **kw)


def _omake(A, oracle_make, case):
    return oracle_make if case[0] == "unicycle" else oracle_of(A, *case[1])


def _gu_step_oracle(A, oracle_make, case, rec):
    def build():
        o = _gu(A, _omake(A, oracle_make, case), case, False, dtype=0 if rec == "f64" else 2)
        o.rollout()
        o.update_expansions()
        o.backward_pass()
        bp = _result(o)
        o.forward_pass()
        return dict(bp=bp, fp=_result(o))
    return _once(("knot giveup step", case, rec), build)


@pytest.mark.parametrize("case,rec", GU_STEP, ids=GU_STEP_IDS)
def test_giveup_step_on_the_oracle(A, oracle_make, case, rec):
    """One backward pass gives up on instances 0 and 2 of every three (status_ilqr 9, regularisation 1e-3) and leaves K and d
    exactly zero on exactly the ks knots below the written ones; the forward pass after it sets the status back to kUnsolved
    and takes a shorter step on an instance that gave up than alpha = 1."""
    ks = case[3]
    r = _gu_step_oracle(A, oracle_make, case, rec)
    st = r["bp"]["stats"]
    gave = np.arange(9) % 3 != 1
    assert (st["status_ilqr"][gave] == A.BACKWARD_PASS_REGULARIZATION_FAILED).all() and (st["regularization"][gave] == 1e-3).all()
    assert (st["status_ilqr"][~gave] == A.UNSOLVED).all() and (st["regularization"][~gave] == 0).all()
    K, d = r["bp"]["K"], r["bp"]["d"]
    zero = ~K.any(axis=(2, 3)) & ~d.any(axis=2)  # [B][N]
    assert zero[gave, :ks].all() and not zero[gave, ks:].any() and not zero[~gave].any()
    fp = r["fp"]["stats"]
    assert (fp["status_ilqr"] == A.UNSOLVED).all() and (fp["alpha"] > 0).all() and (fp["alpha"][gave] < 1).any()
    if case == GU_CASES[0]:
        assert (fp["alpha"][gave] == 0.0625).all() and (fp["alpha"][~gave] == 1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case,rec", GU_STEP, ids=GU_STEP_IDS)
def test_giveup_step(A, oracle_make, hip_make, case, rec):
    """Rollout, expansions and one backward pass that gives up: status and regularisation EXACT, K and d to the step bars and
    exactly zero at every knot the oracle left untouched.  Then the forward pass: alpha and status EXACT, X and U to the bars."""
    model, (n, m), N_, ks = case
    o = _gu_step_oracle(A, oracle_make, case, rec)
    g = _gu(A, hip_make, case, True, dtype=A.F64 if rec == "f64" else A.F32)
    g.rollout()
    g.update_expansions()
    g.backward_pass()
    bp = _result(g)
    tag = f"knot give-up step {model} {n}_{m} N {N_} {rec}"
    _exact(bp["stats"], o["bp"]["stats"], ("status_ilqr", "regularization"), tag)
    untouched = ~o["bp"]["K"].any(axis=(2, 3)) & ~o["bp"]["d"].any(axis=2)
    assert untouched.sum() == 6 * ks
    assert not bp["K"][untouched].any() and not bp["d"][untouched].any(), np.argwhere(bp["K"].any(axis=(2, 3)) & untouched)[:8]
    _ledger.close_normwise(bp["K"], o["bp"]["K"], 1e-9, f"{tag}: K")
    _ledger.close(bp["d"], o["bp"]["d"], STEP_RTOL, STEP_ATOL, f"{tag}: d")
    g.forward_pass()
    fp = _result(g)
    _exact(fp["stats"], o["fp"]["stats"], ("alpha", "status_ilqr"), tag + " forward pass")
    _cmp_step(tag + " forward pass", fp, o["fp"], gains=False)


# ---- 2. give-up, whole solves -------------------------------------------------------------------------------------------------
# (id, case, batch, line_search_max_iterations, per-knot steps)  -- the last two with per-knot steps belong to scenario 5
GU_SOLVES = [(f"{i}-{'ls0' if ls == 0 else 'default'}", c, 9, ls, False) for c, i in zip(GU_CASES, GU_IDS) for ls in (None, 0)]
GU_SOLVES += [("unicycle_3_2-N40-chains", GU_CASES[0], BIG, None, False), ("unicycle_3_2-N40-steps-ls0", GU_CASES[0], 9, 0, True),
              ("chain_5_3-N40-steps-ls0", GU_CASES[2], 9, 0, True)]


def _gu_solve(A, make, case, device, batch, ls, steps):
    opts = dict(max_iterations_inner=6, max_iterations_outer=2)
    if ls is not None:
        opts["line_search_max_iterations"] = ls
    return _gu(A, make, case, device, batch=batch, steps=steps, **opts)


def _gu_solve_oracle(A, oracle_make, case, batch, ls, steps):
    def build():
        o = _threads(_gu_solve(A, _omake(A, oracle_make, case), case, False, batch, ls, steps))
        o.solve()
        return _result(o)
    return _once(("knot giveup solve", case, batch, ls, steps), build)


@pytest.mark.parametrize("cid,case,batch,ls,steps", GU_SOLVES, ids=[c[0] for c in GU_SOLVES])
def test_giveup_solve_on_the_oracle(A, oracle_make, cid, case, batch, ls, steps):
    """Whole solves of GU (6 inner, 2 outer iterations at most): two of every three instances log the capped regularisation;
    with no trial they end with status 9 after one iteration and the others at kMaxInnerIterations; with trials the unicycle at
    N = 40 ends 7 / 6 / 7."""
    st = _gu_solve_oracle(A, oracle_make, case, batch, ls, steps)["stats"]
    gave = np.arange(len(st)) % 3 != 1
    assert (st["regularization"][gave] == 1e-3).all()
    if ls == 0:
        assert (st["status"][gave] == A.BACKWARD_PASS_REGULARIZATION_FAILED).all() and (st["iterations_total"][gave] == 1).all()
        assert (st["status"][~gave] == A.MAX_INNER_ITERATIONS).all() and (st["iterations_total"][~gave] == 6).all()
    else:
        assert (st["status"][gave] == A.MAX_INNER_ITERATIONS).all() and (st["iterations_total"] > 1).all()
        if case == GU_CASES[0]:  # (7 / 6 / 7 at batch 9; over 2050 goals some of the middle third end at kMaxInnerIterations too)
            assert (st["status"][~gave] == A.MAX_OUTER_ITERATIONS).all() if batch == 9 else (st["status"][~gave] == A.MAX_OUTER_ITERATIONS).any()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,case,batch,ls,steps", GU_SOLVES, ids=[c[0] for c in GU_SOLVES])
def test_giveup_solve(A, oracle_make, hip_make, monkeypatch, cid, case, batch, ls, steps):
    """All of SOLVE_FIELDS EXACT; X, U to the bars of whole solves; K and d exactly zero wherever the oracle's are (the knots
    the last backward pass left untouched)."""
    o = _gu_solve_oracle(A, oracle_make, case, batch, ls, steps)
    if batch == BIG:
        for k, v in CHAINS.items():
            monkeypatch.setenv(k, v)
    g = _gu_solve(A, hip_make, case, True, batch, ls, steps)
    g.solve()
    r = _result(g)
    _knot_routed(g)
    _exact(r["stats"], o["stats"], SOLVE_FIELDS, cid)
    _cmp_solve(f"knot give-up solve {cid}", r, o, duals=False)
    untouched = ~o["K"].any(axis=(2, 3)) & ~o["d"].any(axis=2)
    if ls == 0:
        assert untouched.any()
    assert not r["K"][untouched].any() and not r["d"][untouched].any(), np.argwhere(r["K"].any(axis=(2, 3)) & untouched)[:8]


# ---- 3. MO under each option set ------------------------------------------------------------------------------------------------
_st5 = lambda st: _sets(st["status"]).tolist()  # noqa: E731


def _ls40_checks(A, r):
    past20 = [bool((h[h > 0] < 1.2 ** -19.5).any()) for h in r["alpha_history"][:5]]  # (trial t has alpha = 1.2^-t: t >= 20)
    return past20[1:] == [True] * 4 and _st5(r["stats"])[3] == A.MAX_INNER_ITERATIONS and r["stats"]["iterations_total"][3] == 115


# name -> (options, per-knot steps, what the oracle's result must show)
MO_SETS = {
    "default": ({}, False, lambda A, r: _st5(r["stats"]) == [0] * 5 and 17 <= r["stats"]["iterations_total"].min() and r["stats"]["iterations_total"].max() <= 27),
    "maxpen100": (dict(maximum_penalty=100.0), False, lambda A, r: _st5(r["stats"]) == [A.MAX_PENALTY] * 5),
    "maxpen1000": (dict(maximum_penalty=1000.0), False, lambda A, r: _st5(r["stats"]) == [A.MAX_PENALTY, 0, 0, 0, 0]),
    "state2.0": (dict(state_max=2.0), False, lambda A, r: _st5(r["stats"]) == [A.STATE_LIMIT] * 5 and (r["stats"]["iterations_outer"] == 1).all()
                 and 10 <= r["stats"]["iterations_total"].min() and r["stats"]["iterations_total"].max() <= 14),
    "state2.4": (dict(state_max=2.4), False, lambda A, r: _st5(r["stats"]) == [0, 0] + [A.STATE_LIMIT] * 3),
    "control0.8": (dict(control_max=0.8), False, lambda A, r: _st5(r["stats"]) == [A.CONTROL_LIMIT] * 5
                   and _sets(r["stats"]["iterations_outer"]).tolist() == [4, 4, 1, 1, 1]),
    "control0.9": (dict(control_max=0.9), False, lambda A, r: _st5(r["stats"]) == [0, 0, 0] + [A.CONTROL_LIMIT] * 2),
    "control2.0": (dict(control_max=2.0), False, lambda A, r: _st5(r["stats"]) == [0] * 5),
    "caps": (dict(max_iterations_inner=5, max_iterations_outer=4), False, lambda A, r: _st5(r["stats"]) == [A.MAX_INNER_ITERATIONS] * 5),
    "total7": (dict(max_iterations_total=7), False, lambda A, r: _st5(r["stats"]) == [A.MAX_ITERATIONS] * 5 and (r["stats"]["iterations_total"] == 7).all()),
    "ls3": (dict(line_search_max_iterations=3), False, lambda A, r: _st5(r["stats"]) == [0, A.MAX_PENALTY] + [A.MAX_INNER_ITERATIONS] * 3
            and r["stats"]["iterations_total"].min() == 16 and r["stats"]["iterations_total"].max() == 110),
    "ls0": (dict(line_search_max_iterations=0), False, lambda A, r: _st5(r["stats"]) == [A.MAX_INNER_ITERATIONS] * 5 and (r["stats"]["iterations_total"] == 100).all()),
    "ls40": (dict(line_search_max_iterations=40, line_search_decrease_factor=1.2, line_search_lower_bound=0.3), False, _ls40_checks),
    "steps": ({}, True, lambda A, r: _st5(r["stats"]) == [0] * 5 and 28 <= r["stats"]["iterations_total"].min() and r["stats"]["iterations_total"].max() <= 33),
}
MO_BIG = ["ls3", "maxpen1000"]
HISTORY = ("alpha", "max_penalty", "regularization", "cost", "cost_decrease", "gradient", "violations")


def _mo_oracle(P, oracle_make, name):
    """The oracle's solve of MO under MO_SETS[name]: stats, X, U, gains, duals, penalties, the cost-to-go of its last backward
    pass and the history of every instance."""
    def build():
        opts, steps, _ = MO_SETS[name]
        o = C.mo(P, oracle_make, 10, True, steps=steps, **opts)
        o.solve()
        r = _al_result(o)
        r["P"], r["p"] = o.get_ctg()
        r["history"] = {f: [o.get_history(b, f) for b in range(10)] for f in HISTORY}
        r["alpha_history"] = r["history"]["alpha"]
        return r
    return _once(("knot MO", name), build)


@pytest.mark.parametrize("name", list(MO_SETS))
def test_mo_options_on_the_oracle(A, P, oracle_make, name):
    """Each option set takes the oracle where MO_SETS says -- the statuses per parameter set, the iteration counts -- and
    the two instances of a parameter set agree bit for bit (what lets a large batch be compared through b mod 5)."""
    r = _mo_oracle(P, oracle_make, name)
    assert MO_SETS[name][2](A, r), (name, r["stats"][list(MO_FIELDS)])
    for f in ("stats", "X", "U", "lam", "pen"):
        assert r[f][:5].tobytes() == r[f][5:].tobytes(), f
    if name == "control2.0":
        assert not (r["stats"]["status"] == A.CONTROL_LIMIT).any()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MO_SETS))
def test_mo_options(A, P, oracle_make, hip_make, name):
    """status, status_ilqr, the three iteration counts, regularisation, alpha and max_penalty EXACT; X, U, duals and penalties
    to the bars of whole solves."""
    o = _mo_oracle(P, oracle_make, name)
    opts, steps, _ = MO_SETS[name]
    g = C.mo(P, hip_make, 10, False, steps=steps, **opts)
    g.solve()
    r = _al_result(g)
    _knot_routed(g)
    print(f"MO {name}: statuses {_st5(r['stats'])}, iterations {_sets(r['stats']['iterations_total']).tolist()}")
    _exact(r["stats"], o["stats"], MO_FIELDS, f"MO {name}")
    _cmp_solve(f"knot MO {name}", r, o)


@pytest.mark.gpu
@pytest.mark.parametrize("name", MO_BIG)
def test_mo_options_on_four_chains(A, P, oracle_make, hip_make, monkeypatch, name):
    """Batch 2050 on four chains: every instance against the oracle's instance of its parameter set (b mod 5; the oracle's
    instances are independent of each other and test_mo_options_on_the_oracle holds that two of a set agree bit for bit) --
    the exact fields with ==, the values to the bars; and bit for bit against the device's own batch of 10."""
    o = _mo_oracle(P, oracle_make, name)
    opts, steps, _ = MO_SETS[name]
    small = C.mo(P, hip_make, 10, False, steps=steps, **opts)
    small.solve()
    rs = _al_result(small)
    for k, v in CHAINS.items():
        monkeypatch.setenv(k, v)
    g = C.mo(P, hip_make, BIG, False, steps=steps, **opts)
    g.solve()
    r = _al_result(g)
    _knot_routed(g)
    of = np.arange(BIG) % 5
    ob = {f: o[f][of] for f in ("stats", "X", "U", "lam", "pen")}
    _exact(r["stats"], ob["stats"], MO_FIELDS, f"MO {name} batch {BIG}")
    _cmp_solve(f"knot MO {name} batch {BIG}", r, ob)
    for f in ("stats", "X", "U", "K", "d", "lam", "pen"):
        assert r[f].tobytes() == np.ascontiguousarray(rs[f][of]).tobytes(), (name, f)


# ---- 4. the rollout limits at step level ----------------------------------------------------------------------------------------
# The guess is U = (0.2, 0.2) (twice problems.tracking_slalom's): on the oracle the first line search then accepts alpha = 1
# on every instance, the control of knot 0 has the largest norm of that rollout (1.65 .. 1.97 over the sets against 1.04 ..
# 1.34 elsewhere: the correction of the 0.1 the initial state lies off the path) and |x| grows to knot N.  Limits come from
# that unlimited run:
#   u0:   control_max between |u_0| and the other controls over ALL sets, state_max = 2.0, which every set passes at a later
#         knot: step 0 fails on its control, and a check that misses it meets the state limit later (status 2 for 3)
#   xN-p: state_max between |x_N| and the other states of parameter set p: for that set knot N alone is over the limit;
#         the sets below it stay inside, the sets above it are over on earlier knots too
# With the default trials a later trial passes (alpha < 1, kUnsolved); with ONE trial the limit status stays; with the check
# switched off the same inputs give the unlimited run.
GUESS = np.array([0.2, 0.2])
LIMIT_CASES = ["u0", "xN-0", "xN-3"]


def _mo_sweep(P, make, device, **opts):
    s = C.mo(P, make, 10, not device, **opts)
    s.set_trajectory(None, np.tile(GUESS, (N, 1)))
    s.rollout()
    s.update_expansions()
    s.backward_pass()
    s.forward_pass()
    return _result(s, gains=False)


def _limit_opts(P, oracle_make, case):
    def build():
        free = _mo_sweep(P, oracle_make, False)
        xn, un = np.linalg.norm(free["X"], axis=2), np.linalg.norm(free["U"], axis=2)
        assert (free["stats"]["alpha"] == 1.0).all() and (np.diff(xn[:, 1:], axis=1) > 0).all()
        if case == "u0":
            lo, hi = un[:, 1:].max(), un[:, 0].min()
            assert lo < hi and (xn[:, 1] < 2.0).all() and (xn[:, -1] > 2.0).all()
            return dict(control_max=0.5 * (lo + hi), state_max=2.0), free
        p = int(case[-1])
        lo, hi = xn[p, :-1].max(), xn[p, -1]
        assert lo < hi
        return dict(state_max=0.5 * (lo + hi)), free
    return _once(("knot limit opts", case), build)


def _limit_oracle(P, oracle_make, case, how):
    def build():
        opts, _ = _limit_opts(P, oracle_make, case)
        extra = {"trials": {}, "one": dict(line_search_max_iterations=1), "off": dict(line_search_max_iterations=1, check_forwardpass_bounds=0)}[how]
        return _mo_sweep(P, oracle_make, False, **opts, **extra)
    return _once(("knot limit", case, how), build)


@pytest.mark.parametrize("case", LIMIT_CASES)
def test_limit_step_on_the_oracle(A, P, oracle_make, case):
    _, free = _limit_opts(P, oracle_make, case)
    trials, one, off = (_limit_oracle(P, oracle_make, case, how)["stats"] for how in ("trials", "one", "off"))
    hit = np.ones(10, dtype=bool) if case == "u0" else np.arange(10) % 5 >= int(case[-1])
    assert (trials["alpha"][hit] < 1).all() and (trials["alpha"][hit] > 0).all() and (trials["alpha"][~hit] == 1).all()
    assert (trials["status_ilqr"] == A.UNSOLVED).all()
    assert (one["status_ilqr"][hit] == (A.CONTROL_LIMIT if case == "u0" else A.STATE_LIMIT)).all() and (one["alpha"][hit] == 0).all()
    assert (one["status_ilqr"][~hit] == A.UNSOLVED).all() and (one["alpha"][~hit] == 1).all()
    assert (off["status_ilqr"] == A.UNSOLVED).all() and (off["alpha"] == 1).all()
    assert off.tobytes() == free["stats"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("case", LIMIT_CASES)
def test_limit_step(A, P, oracle_make, hip_make, case):
    """One forward pass whose first failing step is the control of knot 0, or the state of knot N: alpha and status_ilqr EXACT
    with the default trials, with one trial (the limit status stays) and with check_forwardpass_bounds = 0 (kUnsolved)."""
    opts, _ = _limit_opts(P, oracle_make, case)
    for how, extra in (("trials", {}), ("one", dict(line_search_max_iterations=1)),
                       ("off", dict(line_search_max_iterations=1, check_forwardpass_bounds=0))):
        o = _limit_oracle(P, oracle_make, case, how)
        r = _mo_sweep(P, hip_make, True, **opts, **extra)
        _exact(r["stats"], o["stats"], ("alpha", "status_ilqr"), f"limit {case} {how}")
        _cmp_step(f"knot limit step {case} {how}", r, o, gains=False)


# ---- 5. per-knot steps ----------------------------------------------------------------------------------------------------------
# (whole solves: MO_SETS["steps"] and the two -steps-ls0 cases of GU_SOLVES)
def _steps_sweep_oracle(P, oracle_make):
    return _once(("knot steps sweep",), lambda: _mo_sweep(P, oracle_make, False, steps=True))


def test_steps_sweep_on_the_oracle(P, oracle_make):
    """Alternating steps change the oracle's first sweep: another trajectory than with the uniform step."""
    a, b = _steps_sweep_oracle(P, oracle_make), _limit_opts(P, oracle_make, "u0")[1]
    assert (a["stats"]["alpha"] > 0).all() and np.abs(a["X"] - b["X"]).max() > 1e-3


@pytest.mark.gpu
def test_steps_sweep(P, oracle_make, hip_make):
    """MO with alternating steps 0.05 / 0.04, one sweep: alpha and status EXACT, X and U to the step bars."""
    o = _steps_sweep_oracle(P, oracle_make)
    r = _mo_sweep(P, hip_make, True, steps=True)
    _exact(r["stats"], o["stats"], ("alpha", "status_ilqr"), "steps sweep")
    _cmp_step("knot steps sweep", r, o, gains=False)


# ---- 6. the history ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["default", "ls3"])
def test_history_on_the_oracle(A, P, oracle_make, name):
    """The oracle's history has a row per iteration and is not flat: alpha takes more than one value, the penalty grows."""
    r = _mo_oracle(P, oracle_make, name)
    for b in range(10):
        assert all(len(r["history"][f][b]) >= r["stats"]["iterations_total"][b] for f in HISTORY)
        assert len(np.unique(r["history"]["alpha"][b])) >= 2 and len(np.unique(r["history"]["max_penalty"][b])) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "ls3"])
def test_history(A, P, oracle_make, hip_make, name):
    """set_record_history on MO: for every instance alpha, max_penalty and regularization EXACT, cost, cost_decrease, gradient
    and violations to the bars of test_parity_gpu.py::test_history_matches_oracle; at least iterations_total rows."""
    o = _mo_oracle(P, oracle_make, name)
    opts, steps, _ = MO_SETS[name]
    g = C.mo(P, hip_make, 10, False, steps=steps, **opts)
    g.set_record_history(301)
    g.solve()
    _exact(g.get_stats(), o["stats"], MO_FIELDS, f"history {name}")
    for b in range(10):
        for f, tol in (("alpha", 0), ("max_penalty", 0), ("regularization", 0), ("cost", 1e-9), ("cost_decrease", 1e-6), ("gradient", 1e-7),
                       ("violations", 1e-7)):
            ho, hg = o["history"][f][b], g.get_history(b, f)
            rows = min(len(ho), len(hg))  # (the reference's vectors end with the row the last NewIteration opened, a copy)
            assert rows >= o["stats"]["iterations_total"][b], (b, f, len(ho), len(hg))
            if tol == 0:
                assert np.array_equal(hg[:rows], ho[:rows]), (b, f, hg[:rows], ho[:rows])
            else:
                _ledger.close(hg[:rows], ho[:rows], tol, 1e-9, f"knot history {name}: {f}")


# ---- 7. the cost-to-go --------------------------------------------------------------------------------------------------------------
def test_ctg_on_the_oracle(P, oracle_make):
    """The oracle's P of the last backward pass is symmetric and definite on every knot, and differs from knot to knot."""
    r = _mo_oracle(P, oracle_make, "default")
    Pt = np.swapaxes(r["P"], 2, 3)
    assert np.abs(r["P"] - Pt).max() < 1e-10 and (np.linalg.eigvalsh(0.5 * (r["P"] + Pt)) > 0).all()
    assert np.abs(np.diff(r["P"], axis=1)).max(axis=(2, 3)).min() > 0 and r["p"].any()


@pytest.mark.gpu
def test_ctg(A, P, oracle_make, hip_make):
    """get_ctg after a whole MO solve (the replay: Engine::ReplayCtg) equals get_ctg of a handle that recorded during the same
    solve, bit for bit, and changes nothing on the handle; both against the oracle's at the step bars.
    What Engine::GetCtg promises once the window has moved: the records belong to the LAST BACKWARD PASS (ctg_fresh_), and a
    read behind a solve that did not record replays that pass only while its inputs are those the solve left
    (ctg_replayable_).  So after set_track_offset or set_reference_offset a handle that holds no records refuses with
    ALTRO_NOT_READY -- no replay over the new window --, and a handle that holds them (recorded, or replayed before the move)
    returns the same bytes as before: the last pass's, not something recomputed.  mpc_advance drops the records with the
    shift: both kinds of handle refuse."""
    o = _mo_oracle(P, oracle_make, "default")
    replay, recorded = C.mo(P, hip_make, 10, False), C.mo(P, hip_make, 10, False)
    recorded.set_record_ctg(True)
    replay.solve()
    recorded.solve()
    before = _al_result(replay)
    Pr, pr = replay.get_ctg()
    Pc, pc = recorded.get_ctg()
    after = _al_result(replay)
    assert Pr.tobytes() == Pc.tobytes() and pr.tobytes() == pc.tobytes()
    for f in before:
        assert before[f].tobytes() == after[f].tobytes(), f
    assert before["stats"].tobytes() == recorded.get_stats().tobytes()
    _ledger.close(Pr, o["P"], STEP_RTOL, STEP_ATOL, "knot ctg: P")
    _ledger.close(pr, o["p"], STEP_RTOL, STEP_ATOL, "knot ctg: p")

    def refused(s):
        with pytest.raises(A.AltroError) as e:
            s.get_ctg()
        assert f"({A.NOT_READY})" in str(e.value) and "cost-to-go" in str(e.value), str(e.value)

    moves = (lambda s: s.set_track_offset(C.OFFSET_MO + 1), lambda s: s.set_reference_offset(C.OFFSET_MO + 1), lambda s: s.mpc_advance(3))
    for move in moves:  # no records held: nothing to read, and no replay
        s = C.mo(P, hip_make, 10, False)
        s.solve()
        move(s)
        refused(s)
    for holder in (replay, recorded):  # records held: the last backward pass's, unchanged by the window
        for move in moves[:2]:
            move(holder)
            Ph, ph = holder.get_ctg()
            assert Ph.tobytes() == Pr.tobytes() and ph.tobytes() == pr.tobytes()
        moves[2](holder)
        refused(holder)


# ---- 8. warm start -----------------------------------------------------------------------------------------------------------------
SHIFT = 3


def _warm_oracle(P, oracle_make):
    def build():
        first = _mo_oracle(P, oracle_make, "default")
        src = M.row_map(N, SHIFT, MOVING_CONS)
        Xn, Un, lam, pen = M.shifted(first["X"], first["U"], first["lam"], first["pen"], src, SHIFT, 1.0)
        o = C.mo(P, oracle_make, 10, True, offset=C.OFFSET_MO + SHIFT, reset_duals=0, initial_penalty=0.0)
        o.set_initial_state(first["X"][:, SHIFT].copy())
        o.set_trajectory(Xn, Un)
        o.set_duals(lam)
        o.set_penalties(pen)
        o.solve()
        r = _al_result(o)
        r["src"], r["pen0"] = src, pen
        return r
    return _once(("knot warm",), build)


def test_warm_start_on_the_oracle(A, P, oracle_make):
    """The second solve starts from carried penalties above 1 (every row of the moved window has a source: both constraints reach
    knot N - 1, where the shift clamps) and ends solved in fewer iterations than the first one."""
    first, r = _mo_oracle(P, oracle_make, "default"), _warm_oracle(P, oracle_make)
    assert (r["src"] >= 0).all() and (r["src"] != np.arange(len(r["src"]))).any() and (r["pen0"] > 1.0).any()
    assert (r["stats"]["status"] == A.SOLVED).all() and (r["stats"]["iterations_total"] < first["stats"]["iterations_total"]).all()
    assert (r["stats"]["iterations_total"] >= 1).all()


@pytest.mark.gpu
def test_warm_start(A, P, oracle_make, hip_make):
    """Solve; reset_duals = 0, initial_penalty = 0; mpc_advance(3); solve.  The oracle takes the advanced window as a fresh
    per-knot problem at offset 8 with its own plan shifted, its duals and penalties carried over through the row map
    (set_duals, set_penalties): statuses and iteration counts EXACT, both solves; values to the bars of whole solves."""
    first, o = _mo_oracle(P, oracle_make, "default"), _warm_oracle(P, oracle_make)
    g = C.mo(P, hip_make, 10, False)
    g.solve()
    _exact(g.get_stats(), first["stats"], MO_FIELDS, "warm start, first solve")
    assert np.array_equal(g.mpc_row_map(SHIFT), o["src"])
    g.set_options(reset_duals=0, initial_penalty=0.0)
    g.mpc_advance(SHIFT)
    assert g.get_track_offset() == g.get_reference_offset() == C.OFFSET_MO + SHIFT
    _ledger.close(g.get_penalties(), o["pen0"], RTOL, 0.0, "knot warm start: penalties carried over")
    g.solve()
    r = _al_result(g)
    _exact(r["stats"], o["stats"], MO_FIELDS, "warm start, second solve")
    _cmp_solve("knot warm start", r, o)
