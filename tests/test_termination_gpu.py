"""The termination paths of the iLQR and AL loops (ilqr.hpp:409-427, 484-495; al_solver.hpp:357-401) on every engine path,
against the oracle.

The HIP code restates these exits per kernel: four backward kernels carry the regularisation give-up, two forward families
check the rollout bounds (k_forward in-lane; k_forward2 / k_sweep_fused / k_sweep_loop through the scalar masks of
BoundMasks), and the AL decision feeds the persistent kernel, the device-side loop and the host-paced sweeps.  Every scenario
has a test without a GPU -- the oracle alone reaches the path, so the GPU test beside it cannot pass vacuously -- and a GPU
test against the oracle:

  1  the regularisation give-up (status 9): indefinite R on knots 0 .. ks-1 only, bp_reg_max = 1e-3, threshold 3.  The
     reference leaves the gains of the failing knot and of every knot below it untouched; the forward pass of the same
     iteration rolls out with them.  One case per backward kernel, with the written knots crossing a gain chunk; whole solves
     on every engine path; the same with no line-search trial at all, the only way status 9 survives a solve
  2  ALTRO_MAX_PENALTY (8)
  3  the rollout limits: final statuses 2 and 3; the first failing step decides (one knot over a limit, at either end of the
     horizon; control before state, state before control, both at one step); the check switched off
  4  options the suite never varied (the list of test_options_gpu.py::test_option_variations): each changes the oracle's
     schedule, or a regularisation that is raised

Found by these tests and fixed with them (each of the give-up tests named fails without its fix):
  - k_backward_mfma / the device loop's backward pass wrote out every counted slot of their LDS gain chunk after a failed
    factorisation: after the give-up the failing knot and the knots below it held other knots' gains (test_giveup_step,
    test_giveup_solve on the batched paths)
  - the persistent kernel stages no gains, so a pass that gave up in the first iteration of a launch rolled out with
    uninitialised LDS at the untouched knots (test_giveup_solve[unicycle-persistent], [chain_1_1-b9])
  - with no line-search trial k_forward reset the status to kUnsolved and k_forward2 took another lane's
    (test_giveup_solve[*-ls0]); the engine now runs that case on the batched kernels, which keep the backward pass's status

kCostIncrease (4) has no test: the reference sets J = J0 before it tests J > J0 (ilqr.hpp:549-557), so the status is
unreachable.

Every scenario here is built from ordinary costs and constraints.  A handle with a tracking cost or a knot constraint
(Engine::KnotRouted) runs none of these kernels but the *_trk twins: tests/test_knot_termination_gpu.py takes the same exits
there.

Engine switches are read when a handle is created: the GPU tests set them before make().  Statuses, iteration counts, alpha
and the regularisation are compared exactly; values go through the ledger (tests/_ledger.py) to bars of ~10x the measured
maxima (profiles/r06_parity_errors.json), never below 1e-14 abs / 1e-13 norm-wise."""
import ctypes
import os

import numpy as np
import pytest

import _ledger
from test_model_shapes_gpu import chain_restart, kind_of, oracle_of, unicycle_restart_mix

# ---- engine paths ---------------------------------------------------------------------------------------------------------
# batch <= 512: the persistent kernel (k_sweep_fused) alone; 513 .. 1536: the device-side loop (k_sweep_loop) and the
# persistent tail; ALTRO_HIP_SWEEP_LOOP=0: host-paced sweeps and the tail; ALTRO_HIP_NO_FUSED_SWEEP=1: the batched sweeps
# alone; batch >= 2048 with four chains of host-paced sweeps
ENGINES = {"persistent": (7, {}), "loop": (640, {}), "sweeps": (640, {"ALTRO_HIP_SWEEP_LOOP": "0"}),
           "batched": (640, {"ALTRO_HIP_NO_FUSED_SWEEP": "1"}), "chains": (2048, {"ALTRO_HIP_CHAINS": "4"})}


def _setenv(monkeypatch, path):
    for k, v in ENGINES[path][1].items():
        monkeypatch.setenv(k, v)


def _threads(s):
    if s.batch > 64:
        s._lib.oracle_set_threads(s._h, ctypes.c_int(min(16, len(os.sched_getaffinity(0)))))
    return s


def alternating(N, a, b):
    """Per-knot steps of two alternating values: the general kernels (k_forward) take the solve."""
    return np.where(np.arange(N) % 2 == 0, np.float32(a), np.float32(b)).astype(np.float32)


_cache = {}


def _once(key, build):
    """The oracle's result of a scenario, computed once and shared by the tests that need it (read only)."""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _result(s, gains=True):
    r = dict(stats=s.get_stats())
    r["X"], r["U"] = s.get_trajectory()
    if gains:
        r["K"], r["d"] = s.get_gains()
    for a in r.values():
        a.setflags(write=False)
    return r


def _exact(sg, so, fields, tag):
    for f in fields:
        assert np.array_equal(sg[f], so[f]), (tag, f, np.flatnonzero(sg[f] != so[f])[:8], sg[f][:9], so[f][:9])


# Bars (GPU against oracle) per family of comparisons (the longest key a comparison's tag starts with): absolute for X, U,
# d, duals and penalties, norm-wise per instance for K; ~10x the maximum measured on the MI355X over the family (in the
# comment beside each; profiles/r06_parity_errors.json has every member), never below 1e-14 abs / 1e-13 norm-wise.  A
# comparison without an entry is held to the bars of the restart tests (test_model_shapes_gpu.py::test_gain_chunk_horizons):
# 1e-9 rel + 1e-11 abs, K 1e-9 norm-wise.
_BARS = {
    "give-up step chain": {"U": 1e-14, "X": 1e-14, "K": 1e-13, "d": 1e-14},  # measured U 3.3e-16, X 2.2e-16, K 1.1e-15, d 1.0e-15
    "give-up step unicycle": {"U": 5e-12, "X": 5e-13, "K": 1e-13, "d": 5e-13},  # measured U 3.1e-13, X 4.4e-14, K 9.4e-15, d 2.8e-14
    "give-up solve chain": {"K": 1e-13, "U": 1e-14, "X": 1e-14, "d": 1e-14},  # measured K 1.6e-15, U 2.5e-16, X 1.7e-16, d 6.1e-16
    "give-up solve unicycle": {"K": 2e-11, "U": 1e-11, "X": 1e-12, "d": 5e-09},  # measured K 1.5e-12, U 8.1e-13, X 9.4e-14, d 2.0e-10
    "restart mix": {"K": 1e-13, "U": 5e-13, "X": 1e-13, "d": 2e-12},  # measured K 6.8e-15, U 2.7e-14, X 7.7e-15, d 1.3e-13
    "limit edge": {"U": 2e-14, "X": 1e-14},  # measured U 1.8e-15, X 4.4e-16
    "limit ": {"K": 5e-13, "U": 1e-14, "X": 1e-14, "d": 1e-10},  # measured K 2.7e-14, U 0.0e+00, X 5.6e-17, d 5.7e-12
    "max penalty": {"U": 5e-12, "X": 5e-13, "duals": 5e-12, "penalties": 1e-14},  # measured U 2.3e-13, X 2.1e-14, duals 2.0e-13, penalties 0.0e+00
    "bounds check off": {"X": 1e-13},  # measured X 6.7e-15
}


def _cmp(tag, qty, g, o):
    fam = max((k for k in _BARS if tag.startswith(k)), key=len, default=None)
    bar = _BARS[fam].get(qty) if fam else None
    if qty == "K":
        _ledger.close_normwise(g, o, bar if bar else 1e-9, f"{tag}: K")
    else:
        _ledger.close(g, o, 0.0 if bar else 1e-9, bar if bar else 1e-11, f"{tag}: {qty}")


def _values(g, o, tag, gains=True):
    for qty in ("X", "U", "K", "d") if gains else ("X", "U"):
        _cmp(tag, qty, g[qty], o[qty])


# ---- 1. the regularisation give-up ----------------------------------------------------------------------------------------
# (model, (n, m), N, ks): one per backward kernel -- the 4 x 4 MFMA kernel (built-in unicycle and the (1,1) chain, whose
# gain record has another stride), k_backward_mfma16, k_backward_coop, the VALU kernel.  The written knots ks .. N-1 cross a
# gain chunk (kBwdChunk = 126, kM16Chunk = 32) and the failing knot ks-1 lies inside the second one.
GIVEUP = [("unicycle", (3, 2), 160, 20), ("chain", (1, 1), 160, 20), ("chain", (5, 3), 40, 4), ("chain", (6, 5), 40, 4),
          ("chain", (3, 5), 40, 4)]
GIVEUP_IDS = [f"{mo}_{n}_{m}" for mo, (n, m), _, _ in GIVEUP]
GIVEUP_F32 = [GIVEUP[0], GIVEUP[2]]
GIVEUP_OPTS = dict(bp_reg_max=1e-3, bp_reg_fail_threshold=3)


def giveup_problem(A, make, kind, model, shape, N, ks, batch, dtype=0, steps=None, **opts):
    """The restart mix with the indefinite R on knots 0 .. ks-1 only: the sweep passes knots N-1 .. ks, fails at ks-1, and
    with bp_reg_max = 1e-3 gives up after three increases.  Instances 1, 4, 7 ... start outside their control bounds: the
    penalty makes their Quu definite and they pass."""
    n, m = shape
    if model == "unicycle":
        s = unicycle_restart_mix(A, make, batch, N, dtype)
        xf = np.tile(np.array([1.0, 0.5, 0.3]), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
    else:
        s = chain_restart(A, make, kind, n, m, batch=batch, N=N, dtype=dtype, mix=True)
        xf = np.tile(0.3 + 0.1 * np.arange(n), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
    s.set_lqr_cost(ks, N, np.eye(n) * 1e-3, np.eye(m) * 1e-3, xf, np.zeros(m))
    if steps is not None:
        s.set_steps(steps)
    s.set_options(**dict(GIVEUP_OPTS, **opts))
    return s


def _omake(A, oracle_make, model, shape):
    return oracle_make if model == "unicycle" else oracle_of(A, *shape)


def _giveup_step_oracle(A, oracle_make, case, odtype):
    """rollout; update_expansions; backward_pass -> 'bp'; forward_pass -> 'fp' (batch 9)."""
    model, shape, N, ks = case

    def build():
        o = giveup_problem(A, _omake(A, oracle_make, model, shape), A.MODEL_USER_BASE, model, shape, N, ks, 9, odtype)
        o.rollout()
        o.update_expansions()
        o.backward_pass()
        bp = _result(o)
        o.forward_pass()
        return dict(bp=bp, fp=_result(o))
    return _once(("giveup step", case, odtype), build)


@pytest.mark.parametrize("case", GIVEUP, ids=GIVEUP_IDS)
def test_giveup_step_on_the_oracle(A, oracle_make, case):
    """The oracle gives up on instances 0 and 2 of every three, with the gains of knots ks .. N-1 written and those of the
    failing knot ks-1 and below exactly zero; the rollout of the forward pass sets the status back to kUnsolved."""
    model, shape, N, ks = case
    for odtype in (0, 2) if case in GIVEUP_F32 else (0,):
        r = _giveup_step_oracle(A, oracle_make, case, odtype)
        st = r["bp"]["stats"]
        gave = np.arange(9) % 3 != 1
        assert (st["status_ilqr"][gave] == A.BACKWARD_PASS_REGULARIZATION_FAILED).all() and (st["regularization"][gave] == 1e-3).all()
        assert (st["status_ilqr"][~gave] == A.UNSOLVED).all() and (st["regularization"][~gave] == 0).all()
        K, d = r["bp"]["K"], r["bp"]["d"]
        assert not K[gave, :ks].any() and not d[gave, :ks].any()
        assert (np.abs(K[:, ks:]).max(axis=(2, 3)) > 0).all() and (np.abs(K[~gave]).max(axis=(2, 3)) > 0).all()
        assert (r["fp"]["stats"]["status_ilqr"] == A.UNSOLVED).all()
        assert (r["fp"]["stats"]["alpha"][gave] > 0).any()  # the partial gains move the trajectory


def _giveup_step_cases():
    return [(c, "f64") for c in GIVEUP] + [(c, "f32") for c in GIVEUP_F32]


@pytest.mark.gpu
@pytest.mark.parametrize("case,rec", _giveup_step_cases(), ids=[f"{mo}_{n}_{m}-{r}" for (mo, (n, m), _, _), r in _giveup_step_cases()])
def test_giveup_step(A, oracle_make, hip_make, case, rec):
    """One backward pass that gives up: status and regularisation EXACT, K and d to the bars and exactly zero at every knot
    the oracle left untouched (the failing knot included) -- a kernel that writes out what its gain buffer held for those
    knots fails here.  Then the forward pass of the same iteration: alpha and status EXACT, X and U to the bars."""
    model, shape, N, ks = case
    o = _giveup_step_oracle(A, oracle_make, case, 0 if rec == "f64" else 2)
    kind = A.MODEL_UNICYCLE if model == "unicycle" else kind_of(A, *shape)
    g = giveup_problem(A, hip_make, kind, model, shape, N, ks, 9, A.F64 if rec == "f64" else A.F32)
    g.rollout()
    g.update_expansions()
    g.backward_pass()
    bp = _result(g)
    tag = f"give-up step {model} {shape[0]}_{shape[1]} {rec}"
    _exact(bp["stats"], o["bp"]["stats"], ("status_ilqr", "regularization"), tag)
    untouched = ~o["bp"]["K"].any(axis=(2, 3)) & ~o["bp"]["d"].any(axis=2)  # [B][N]
    print(f"{tag}: |K|, |d| max at the knots the oracle left untouched: {np.abs(bp['K'][untouched]).max():.3e}, "
          f"{np.abs(bp['d'][untouched]).max():.3e}")
    assert not bp["K"][untouched].any() and not bp["d"][untouched].any(), np.argwhere(bp["K"].any(axis=(2, 3)) & untouched)[:8]
    _cmp(tag, "K", bp["K"], o["bp"]["K"])
    _cmp(tag, "d", bp["d"], o["bp"]["d"])
    g.forward_pass()
    fp = _result(g)
    _exact(fp["stats"], o["fp"]["stats"], ("alpha", "status_ilqr"), tag + " forward pass")
    _values(fp, o["fp"], tag + " forward pass", gains=False)


# whole solves: (id, case, engine path, per-knot steps, line_search_max_iterations)
# (the unicycle's 160 knots do not fit the LDS of the persistent kernels -- 20 candidates of every knot: the engine runs that
#  horizon with the batched kernels, whose backward pass is the one that buffers the gains in chunks, at every batch size.
#  The persistent kernel, the device loop and the host-paced sweeps in front of the persistent tail run N = 100.)
GIVEUP_SHORT = ("unicycle", (3, 2), 100, 20)


def _giveup_solve_cases():
    uni = GIVEUP[0]
    cases = [(f"unicycle-{p}", GIVEUP_SHORT if p in ("persistent", "loop", "sweeps") else uni, p, False, None) for p in ENGINES]
    cases += [("unicycle-N160-b7", uni, None, False, None)]
    cases += [(f"{mo}_{n}_{m}-b9", c, None, False, None) for c in GIVEUP[1:] for mo, (n, m) in [c[:2]]]
    cases += [("unicycle-steps", uni, None, True, None)]
    # no line-search trial at all: persistent kernel, device loop, general kernels
    # (batch 7 and 640: the sizes of the persistent kernel and of the device loop, which the engine leaves to the batched
    #  kernels when there is no trial)
    cases += [("unicycle-b7-ls0", GIVEUP_SHORT, "persistent", False, 0), ("unicycle-b640-ls0", GIVEUP_SHORT, "loop", False, 0),
              ("unicycle-steps-ls0", uni, None, True, 0)]
    return cases


GIVEUP_SOLVES = _giveup_solve_cases()
SOLVE_FIELDS = ("status", "status_ilqr", "iterations_total", "iterations_outer", "iterations_inner", "regularization")


def _giveup_solve(A, make, kind, case, path, steps, ls):
    model, shape, N, ks = case
    batch = ENGINES[path][0] if path else 9
    opts = dict(max_iterations_inner=6, max_iterations_outer=2)
    if ls is not None:
        opts["line_search_max_iterations"] = ls
    s = giveup_problem(A, make, kind, model, shape, N, ks, batch, steps=alternating(N, 0.05, 0.04) if steps else None, **opts)
    return s


def _giveup_solve_oracle(A, oracle_make, case, path, steps, ls):
    def build():
        model, shape = case[:2]
        o = _threads(_giveup_solve(A, _omake(A, oracle_make, model, shape), A.MODEL_USER_BASE, case, path, steps, ls))
        o.solve()
        return _result(o)
    return _once(("giveup solve", case, ENGINES[path][0] if path else 9, steps, ls), build)


@pytest.mark.parametrize("cid,case,path,steps,ls", GIVEUP_SOLVES, ids=[c[0] for c in GIVEUP_SOLVES])
def test_giveup_solve_on_the_oracle(A, oracle_make, cid, case, path, steps, ls):
    """Whole solves of the give-up problem on the oracle: two of every three instances log the capped regularisation; with
    no line-search trial they end with status 9 after one iteration, the others at kMaxInnerIterations."""
    st = _giveup_solve_oracle(A, oracle_make, case, path, steps, ls)["stats"]
    gave = np.arange(len(st)) % 3 != 1
    if ls == 0:
        assert (st["status"][gave] == A.BACKWARD_PASS_REGULARIZATION_FAILED).all() and (st["iterations_total"][gave] == 1).all()
        assert (st["status"][~gave] == A.MAX_INNER_ITERATIONS).all()
    else:
        assert (st["regularization"][gave] == 1e-3).all(), st["regularization"][:9]
        assert (st["iterations_total"] > 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,case,path,steps,ls", GIVEUP_SOLVES, ids=[c[0] for c in GIVEUP_SOLVES])
def test_giveup_solve(A, oracle_make, hip_make, monkeypatch, cid, case, path, steps, ls):
    """Whole solves (6 inner, 2 outer iterations at most) whose backward passes give up, on every engine path, on the
    chains' backward kernels and on the general kernels (per-knot steps): schedule and regularisation EXACT, X, U, K, d to the
    bars.  line_search_max_iterations = 0: the forward pass runs no rollout and the status stays 9."""
    model, shape = case[:2]
    o = _giveup_solve_oracle(A, oracle_make, case, path, steps, ls)
    if path:
        _setenv(monkeypatch, path)
    kind = A.MODEL_UNICYCLE if model == "unicycle" else kind_of(A, *shape)
    g = _giveup_solve(A, hip_make, kind, case, path, steps, ls)
    g.solve()
    r = _result(g)
    if ls != 0:
        _check_path(g, path)
    _exact(r["stats"], o["stats"], SOLVE_FIELDS, cid)
    _values(r, o, f"give-up solve {cid}")


def _check_path(g, path):
    """The engine path the case is about really ran."""
    tm = g.get_timing()
    if path == "persistent":
        assert tm["fused_sweeps"] > 0 and tm["loop_iterations"] == 0
    elif path == "loop":
        assert tm["loop_iterations"] > 0
    elif path == "sweeps":
        assert tm["loop_iterations"] == 0
    elif path in ("batched", "chains"):
        assert tm["loop_iterations"] == 0 and (path == "chains" or tm["fused_sweeps"] == 0)


def _raised_problem(A, make, factor):
    s = unicycle_restart_mix(A, make, 7, 160)
    s.set_options(max_iterations_inner=3, max_iterations_outer=1, **({} if factor is None else dict(bp_reg_increase_factor=factor)))
    return s


def _raised_oracle(A, oracle_make, factor):
    def build():
        o = _raised_problem(A, oracle_make, factor)
        o.solve()
        return _result(o)
    return _once(("raised", factor), build)


def test_increase_factor_on_the_oracle(A, oracle_make):
    """bp_reg_increase_factor only shows where the regularisation is raised: on the restart mix it changes what the oracle
    logs (on batch_turn90 it changes nothing, with or without bp_reg_initial)."""
    a, b = _raised_oracle(A, oracle_make, None)["stats"], _raised_oracle(A, oracle_make, 2.5)["stats"]
    assert (a["regularization"] > 1e-8).any() and (a["regularization"] != b["regularization"]).any()


@pytest.mark.gpu
def test_increase_factor(A, oracle_make, hip_make):
    """The restart mix with bp_reg_increase_factor = 2.5: the regularisation EXACT, the rest as test_gain_chunk_horizons."""
    o = _raised_oracle(A, oracle_make, 2.5)
    g = _raised_problem(A, hip_make, 2.5)
    g.solve()
    r = _result(g)
    _exact(r["stats"], o["stats"], SOLVE_FIELDS, "increase factor")
    _values(r, o, "restart mix, bp_reg_increase_factor 2.5")


# ---- 2. ALTRO_MAX_PENALTY ---------------------------------------------------------------------------------------------------
PENALTY_PATHS = ["persistent", "loop", "sweeps"]


def _turn90(P, make, batch, steps=None, **opts):
    s = P.batch_turn90(make, batch=batch)
    if steps is not None:
        s.set_steps(steps)
    s.set_options(**opts)
    return s


def _al_result(s):
    r = _result(s)
    r["lam"], r["pen"] = s.get_duals(), s.get_penalties()
    return r


def _penalty_oracle(P, oracle_make, batch):
    def build():
        o = _threads(_turn90(P, oracle_make, batch, constraint_tolerance=1e-9, maximum_penalty=50.0))
        o.solve()
        return _al_result(o)
    return _once(("max penalty", batch), build)


@pytest.mark.parametrize("path", PENALTY_PATHS)
def test_max_penalty_on_the_oracle(A, P, oracle_make, path):
    st = _penalty_oracle(P, oracle_make, 6 if path == "persistent" else 640)["stats"]
    assert (st["status"] == A.MAX_PENALTY).all() and (st["iterations_outer"] == 3).all() and (st["max_penalty"] == 100.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PENALTY_PATHS)
def test_max_penalty(A, P, oracle_make, hip_make, monkeypatch, path):
    """al_solver.hpp:380-384: the penalty passes maximum_penalty before the constraints meet a tolerance of 1e-9.  Status,
    iteration counts and max_penalty EXACT; trajectories, penalties and duals to the bars."""
    batch = 6 if path == "persistent" else 640
    o = _penalty_oracle(P, oracle_make, batch)
    _setenv(monkeypatch, path)
    g = _turn90(P, hip_make, batch, constraint_tolerance=1e-9, maximum_penalty=50.0)
    g.solve()
    r = _al_result(g)
    _check_path(g, path)
    _exact(r["stats"], o["stats"], SOLVE_FIELDS[:5] + ("max_penalty",), f"max penalty {path}")
    _values(r, o, f"max penalty {path}", gains=False)
    _cmp(f"max penalty {path}", "penalties", r["pen"], o["pen"])
    _cmp(f"max penalty {path}", "duals", r["lam"], o["lam"])


# ---- 3a. rollout limits: the final status ------------------------------------------------------------------------------------
# (id, options, status, batch / engine path, per-knot steps)
_CTRL = dict(control_max=0.5, line_search_max_iterations=3)
_STATE = dict(state_max=1e-3, max_iterations_inner=3, max_iterations_outer=1)
LIMITS = [("control-" + p, _CTRL, 3, p, False) for p in PENALTY_PATHS] + [("control-steps", _CTRL, 3, None, True),
                                                                        ("state-loop", _STATE, 2, "loop", False),
                                                                        ("state-steps", _STATE, 2, None, True)]


def _limit_batch(path):
    return 6 if path in (None, "persistent") else 640


def _limit_oracle(P, oracle_make, opts, path, steps):
    def build():
        o = _threads(_turn90(P, oracle_make, _limit_batch(path), alternating(100, 0.03, 0.025) if steps else None, **opts))
        o.solve()
        return _result(o)
    return _once(("limit", tuple(sorted(opts.items())), _limit_batch(path), steps), build)


@pytest.mark.parametrize("lid,opts,status,path,steps", LIMITS, ids=[c[0] for c in LIMITS])
def test_limit_status_on_the_oracle(P, oracle_make, lid, opts, status, path, steps):
    st = _limit_oracle(P, oracle_make, opts, path, steps)["stats"]
    assert (st["status"] == status).all() and (st["iterations_total"] == 1).all() and (st["alpha"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lid,opts,status,path,steps", LIMITS, ids=[c[0] for c in LIMITS])
def test_limit_status(P, oracle_make, hip_make, monkeypatch, lid, opts, status, path, steps):
    """Every trial of the first line search leaves control_max (status 3, REQUIRED) or state_max (2): persistent kernel,
    device loop, host-paced sweeps, and k_forward (per-knot steps)."""
    o = _limit_oracle(P, oracle_make, opts, path, steps)
    if path:
        _setenv(monkeypatch, path)
    g = _turn90(P, hip_make, _limit_batch(path), alternating(100, 0.03, 0.025) if steps else None, **opts)
    g.solve()
    r = _result(g)
    assert (r["stats"]["status"] == status).all()
    _exact(r["stats"], o["stats"], SOLVE_FIELDS[:5] + ("alpha",), lid)
    _values(r, o, f"limit {lid}")


# ---- 3b. rollout limits: the first failing step decides ---------------------------------------------------------------------
# Unicycle, N = 33 (odd: the persistent kernel's auxiliary wave checks the knots in pairs), from rest with zero controls.  R
# is large and Q small, so the feedforward step is u_k ~ uref_k and the trial with alpha = 1 rolls out U ~ uref, the one
# with alpha = 0.5 half of it: a uref that stands out at one knot puts that knot alone over a limit chosen between the
# offending norm and the next largest of an UNLIMITED oracle run, and the next trial passes.  A check that misses the knot
# accepts alpha = 1; the statuses need every trial to fail, which one trial per line search arranges.
EDGE_N = 33
EDGE_B = 5


def _uconst(v, w):
    return np.tile(np.array([v, w], dtype=np.float64), (EDGE_N, 1))


def _edge_urefs():
    N = EDGE_N
    e = {}
    u = _uconst(0.2, 0.1)
    u[0] = (1.0, 0.5)
    e["u_0"] = (u, (0, 0, 0))
    u = _uconst(0.2, 0.1)
    u[N - 1] = (1.0, 0.5)
    e["u_N-1"] = (u, (0, 0, 0))
    e["x_N"] = (_uconst(1.0, 0.2), (0, 0, 0))              # the norm of the state grows along the horizon
    u = _uconst(0.0, 0.0)
    u[0], u[1] = (0.0, 10.0), (0.0, -10.0)                  # a turn on the spot and back: theta_1 = 0.5 stands alone
    e["x_1"] = (u, (0.3, 0, 0))                             # (|x| = 0.3 elsewhere: half the turn stays under the midpoint)
    e["x_0"] = (_uconst(-1.0, 0.0), (1.0, 0, 0))           # towards the origin: x_0 has the largest norm
    for name, j in (("u_then_x", 5), ("x_then_u", 25), ("same_step", 15)):
        u = _uconst(0.5, 0.1)                               # forward: |x| grows; control j stands out
        u[j] = (1.5, 0.3)
        e[name] = (u, (0, 0, 0))
    return e


EDGES = _edge_urefs()
EDGE_STATE_FROM = {"u_then_x": 21, "x_then_u": 11, "same_step": 16}  # first knot whose state is over state_max
EDGE_STATUS = {"u_then_x": 3, "x_then_u": 2, "same_step": 2}


def edge_problem(A, make, name, steps, **opts):
    uref, x0 = EDGES[name]
    N, B = EDGE_N, EDGE_B
    s = make(3, 2, N, B, A.F64)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(np.float32(0.05))
    if steps:
        s.set_steps(alternating(N, 0.05, 0.04))
    scale = 1.0 + 0.002 * np.arange(B)[:, None]  # (instances differ a little; one limit has to separate them all)
    k0 = 0
    for k in range(1, N + 1):  # one cost per stretch of knots with the same uref (the engine holds 8 distinct costs)
        if k == N or (uref[k] != uref[k0]).any():
            s.set_lqr_cost(k0, k, np.eye(3) * 1e-3, np.eye(2) * 10.0, np.zeros(3), scale * uref[k0][None, :])
            k0 = k
    s.set_lqr_cost(N, N + 1, np.eye(3) * 1e-3, np.zeros((2, 2)), np.zeros(3), np.zeros(2))
    s.set_initial_state(np.asarray(x0, dtype=np.float64))
    s.set_trajectory(None, np.zeros((N, 2)))
    s.set_options(**opts)
    return s


def _one_sweep(s):
    s.rollout()
    s.update_expansions()
    s.backward_pass()
    s.forward_pass()
    return _result(s, gains=False)


def _between(inside, outside):
    """A limit between the largest norm that has to stay inside and the smallest that has to be over, over the batch."""
    lo, hi = float(np.max(inside)), float(np.min(outside))
    assert lo < hi, (lo, hi)
    return 0.5 * (lo + hi)


def _edge_limits(A, oracle_make, name, steps):
    """(options with the limits, the unlimited oracle result): the limits come from the unlimited run's alpha = 1 rollout."""
    def build():
        free = _one_sweep(edge_problem(A, oracle_make, name, steps))
        assert (free["stats"]["alpha"] == 1.0).all()
        xn, un = np.linalg.norm(free["X"], axis=2), np.linalg.norm(free["U"], axis=2)  # [B][N+1], [B][N]
        opts = {}
        if name in ("u_0", "u_N-1"):
            j = 0 if name == "u_0" else EDGE_N - 1
            opts["control_max"] = _between(np.delete(un, j, axis=1), un[:, j])
        elif name in ("x_N", "x_1"):
            j = EDGE_N if name == "x_N" else 1
            opts["state_max"] = _between(np.delete(xn, [0, j], axis=1), xn[:, j])
        elif name == "x_0":
            opts["state_max"] = _between(xn[:, 1:], xn[:, 0])
        else:
            j = int(np.argmax(un[0]))
            i = EDGE_STATE_FROM[name]
            assert (np.diff(xn, axis=1) > 0).all()  # |x| grows: the states over the limit are x_i .. x_N
            opts["control_max"] = _between(np.delete(un, j, axis=1), un[:, j])
            opts["state_max"] = _between(xn[:, :i], xn[:, i:])
            opts["line_search_max_iterations"] = 1
            # the first failing step: step k checks x_{k+1}, then u_k
            first = min(j, i - 1)
            assert EDGE_STATUS[name] == (2 if i - 1 <= j else 3) and first >= 0
        return opts, free
    return _once(("edge limits", name, steps), build)


def _edge_oracle(A, oracle_make, name, steps, how):
    def build():
        opts, _ = _edge_limits(A, oracle_make, name, steps)
        if how == "step":
            return _one_sweep(edge_problem(A, oracle_make, name, steps, **opts))
        o = edge_problem(A, oracle_make, name, steps, max_iterations_inner=2, max_iterations_outer=1, **opts)
        o.solve()
        return _result(o, gains=False)
    return _once(("edge", name, steps, how), build)


EDGE_CASES = [(name, steps) for name in EDGES for steps in (False, True)]
EDGE_IDS = [f"{name}-{'steps' if steps else 'uniform'}" for name, steps in EDGE_CASES]


@pytest.mark.parametrize("name,steps", EDGE_CASES, ids=EDGE_IDS)
def test_limit_edges_on_the_oracle(A, oracle_make, name, steps):
    """Each construction changes what the oracle does against the unlimited run -- alpha 1 -> 0.5 where one knot is over, the
    status where every trial fails -- except x_0, which is over state_max and never checked."""
    _, free = _edge_limits(A, oracle_make, name, steps)
    st = _edge_oracle(A, oracle_make, name, steps, "step")["stats"]
    if name == "x_0":
        assert (st["alpha"] == 1.0).all() and (st["status_ilqr"] == A.UNSOLVED).all()
    elif name in EDGE_STATUS:
        assert (st["status_ilqr"] == EDGE_STATUS[name]).all() and (free["stats"]["status_ilqr"] == A.UNSOLVED).all()
        assert (_edge_oracle(A, oracle_make, name, steps, "solve")["stats"]["status"] == EDGE_STATUS[name]).all()
    else:
        assert (st["alpha"] == 0.5).all() and (st["status_ilqr"] == A.UNSOLVED).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,steps", EDGE_CASES, ids=EDGE_IDS)
def test_limit_edges(A, oracle_make, hip_make, name, steps):
    """The edges of the bound check on both forward families (uniform steps: k_forward2 at step level and the persistent
    kernel in the solve, both through BoundMasks; per-knot steps: k_forward's in-lane check): alpha and statuses EXACT."""
    opts, _ = _edge_limits(A, oracle_make, name, steps)
    o = _edge_oracle(A, oracle_make, name, steps, "step")
    r = _one_sweep(edge_problem(A, hip_make, name, steps, **opts))
    _exact(r["stats"], o["stats"], ("alpha", "status_ilqr"), f"{name} step")
    _values(r, o, f"limit edge {name}{' steps' if steps else ''}, one sweep", gains=False)
    o = _edge_oracle(A, oracle_make, name, steps, "solve")
    g = edge_problem(A, hip_make, name, steps, max_iterations_inner=2, max_iterations_outer=1, **opts)
    g.solve()
    r = _result(g, gains=False)
    _exact(r["stats"], o["stats"], SOLVE_FIELDS[:5] + ("alpha",), f"{name} solve")
    _values(r, o, f"limit edge {name}{' steps' if steps else ''}, solve", gains=False)


# ---- 3c. the bounds check switched off --------------------------------------------------------------------------------------
def _nocheck_oracle(P, oracle_make, **opts):
    def build():
        o = _turn90(P, oracle_make, 12, **opts)
        o.solve()
        return _result(o)
    return _once(("nocheck", tuple(sorted(opts.items()))), build)


_TINY = dict(state_max=1e-3, control_max=1e-3)


def test_bounds_check_off_on_the_oracle(P, oracle_make):
    """With limits of 1e-3 every rollout fails -- unless check_forwardpass_bounds = 0, which gives the default solve."""
    base, off, on = (_nocheck_oracle(P, oracle_make, **kw) for kw in ({}, dict(check_forwardpass_bounds=0, **_TINY), _TINY))
    assert (on["stats"]["status"] == 2).all()
    assert np.array_equal(off["stats"], base["stats"]) and np.array_equal(off["X"], base["X"]) and np.array_equal(off["U"], base["U"])


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [False, True], ids=["uniform", "steps"])
def test_bounds_check_off(P, oracle_make, hip_make, steps):
    """check_forwardpass_bounds = 0 switches the check off: limits of 1e-3 change nothing, bit for bit, on both forward
    families; and the solve is the oracle's default one."""
    st = alternating(100, 0.03, 0.025) if steps else None
    a = _turn90(P, hip_make, 12, st)
    b = _turn90(P, hip_make, 12, st, check_forwardpass_bounds=0, **_TINY)
    a.solve()
    b.solve()
    ra, rb = _result(a), _result(b)
    assert np.array_equal(ra["stats"], rb["stats"])
    for f in ("X", "U", "K", "d"):
        assert np.array_equal(ra[f], rb[f]), f
    if not steps:
        o = _nocheck_oracle(P, oracle_make)
        _exact(rb["stats"], o["stats"], SOLVE_FIELDS[:5], "bounds check off")
        ok = o["stats"]["status"] == 0
        _cmp("bounds check off, solved instances", "X", rb["X"][ok], o["X"][ok])


# ---- 4. options the suite never varied ---------------------------------------------------------------------------------------
# (the GPU side is test_options_gpu.py::test_option_variations, whose list carries the same entries)
NEW_VARIATIONS = [dict(bp_reg_min=1e-6), dict(bp_reg_increase_factor=2.5, bp_reg_initial=1e-3), dict(line_search_lower_bound=0.2),
                  dict(line_search_upper_bound=1.0), dict(line_search_upper_bound=1.05)]


def _variation_oracle(P, oracle_make, kw):
    def build():
        o = P.batch_turn90(oracle_make, batch=12)
        o.set_record_history(301)
        o.set_options(**kw)
        o.solve()
        return o.get_stats(), [o.get_history(b, "alpha").tolist() for b in range(12)]
    return _once(("variation", tuple(sorted(kw.items()))), build)


@pytest.mark.parametrize("kw", NEW_VARIATIONS, ids=["-".join(kw) for kw in NEW_VARIATIONS])
def test_new_option_variations_change_the_oracle_schedule(P, oracle_make, kw):
    """Each new entry of test_option_variations changes the oracle's schedule on at least one instance of batch_turn90(12)
    (the iteration counts or the history of alpha): none of them is a variation in name only.  (bp_reg_increase_factor by
    itself changes nothing there -- no regularisation is raised; test_increase_factor covers it.)"""
    import test_options_gpu
    listed = [m.args[1] for m in test_options_gpu.test_option_variations.pytestmark if m.name == "parametrize"][0]
    assert kw in listed
    (s0, h0), (s1, h1) = _variation_oracle(P, oracle_make, {}), _variation_oracle(P, oracle_make, kw)
    assert (s0["iterations_total"] != s1["iterations_total"]).any() or any(a != b for a, b in zip(h0, h1))
