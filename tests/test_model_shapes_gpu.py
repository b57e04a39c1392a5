"""The solver kernels across model shapes (n, m) against the oracle compiled from the same model text.

tests/models/shape_chain.hpp is one nonlinear user model whose n and m come from defines; __graft_entry__.SHAPES lists
the shapes, one per branch of the backward dispatch (altro_engine.hpp, LaunchBackward / FusedOk / the LDS plans):

  (1,1) (2,2) (1,2) (3,1)  k_backward_mfma (4 x 4 tiles) + k_sweep_fused + k_sweep_loop.  (1,1) and (2,2) pad the gain
                           record differently in fp32 and fp64 (2 / 4 and 6 / 8 elements): they did not compile before the
                           4 x 4 kernel's LDS gain chunk took the stored record's stride
  (5,3) (7,3) (9,1)        k_backward_mfma16, last row chunk 1/4, 3/4, 1/4 full; m = 3 is the only 3 x 3 Cholesky;
                           n m >= 12 makes the forward pass eligible for the kSrcKdg variant
  (13,2) (6,5)             k_backward_coop (beyond the 16 x 16 tile; m > 4)
  (3,5)                    k_backward (the one-lane-per-instance VALU kernel), n <= 3 with m > 2

The knot-routed twins of the expansion, forward and cost kernels (tracking costs, knot constraints) run the same ten shapes
in tests/test_knot_shapes_gpu.py.

Every comparison lands in the ledger (tests/_ledger.py) next to its bar."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import _ledger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SHAPES = list(graft.SHAPES)
MFMA4 = [s for s in SHAPES if s[0] <= 3 and s[1] <= 2]
MFMA16 = [s for s in SHAPES if 4 <= s[0] <= 12 and s[1] <= 4]
COOP = [s for s in SHAPES if s not in MFMA4 and s not in MFMA16 and s[0] >= 6]
F32_SHAPES = [(1, 1), (2, 2), (5, 3), (3, 5), (13, 2)]


def ids(shapes):
    return [f"{n}_{m}" for n, m in shapes]


# Problem builders, shared with the child processes of the kernel-agreement tests (the backward kernel and the launch
# variants are chosen when an engine is created, from the environment).
def chain_rk4(X0, U, h, n, m):
    """Rollout of tests/models/shape_chain.hpp (RK4) in numpy: the goals are states the chain reaches."""
    def f(x, u):
        xd = -0.1 * np.sin(x)
        xd[:, :-1] += x[:, 1:]
        for j in range(m):
            xd[:, n - 1 - j % n] += (1.0 + 0.1 * j) * u[:, j]
        return xd
    x = X0.copy()
    for k in range(U.shape[1]):
        u = U[:, k]
        k1 = f(x, u)
        k2 = f(x + 0.5 * h * k1, u)
        k3 = f(x + 0.5 * h * k2, u)
        k4 = f(x + h * k3, u)
        x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def chain_goals(n, m, N, batch, seed=0):
    """Seeded, jittered goals: where constant controls of up to +-0.5 lead the chain from rest in N knots."""
    rng = np.random.default_rng(1000 * n + 10 * m + seed)
    u = rng.uniform(-0.5, 0.5, (batch, 1, m))
    return chain_rk4(np.zeros((batch, n)), np.broadcast_to(u, (batch, N, m)), 0.05, n, m)


# control bound of each shape: active on part of the batch (on the oracle, batch 24: 4 - 96 % of the instances), well
# clear of the 100+ iteration stragglers a tighter bound makes
BOUND = {(5, 3): 3.0, (6, 5): 3.0, (3, 5): 3.0, (9, 1): 0.5}


def chain_al(A, make, kind, n, m, batch, N=60, dtype=0, seed=0):
    """AL problem: reach a jittered goal (goal constraint) under control bounds that are active on part of the batch."""
    bound = BOUND.get((n, m), 2.0)
    s = make(n, m, N, batch, dtype)
    h = np.float32(0.05)
    hd = float(h)
    xf = chain_goals(n, m, N, batch, seed)
    s.set_model(kind)
    s.set_uniform_step(h)
    s.set_lqr_cost(0, N, np.eye(n) * (0.1 * hd), np.eye(m) * (1e-2 * hd), xf, np.zeros(m))
    s.set_lqr_cost(N, N + 1, np.eye(n) * 10.0, np.zeros((m, m)), xf, np.zeros(m))
    s.add_control_bound(0, N, [-bound] * m, [bound] * m)
    s.add_constraint(A.CON_GOAL, N, N + 1, xf)
    s.set_initial_state(np.zeros(n))
    s.set_trajectory(None, np.zeros((N, m)))
    return s


def chain_restart(A, make, kind, n, m, batch, N=40, dtype=0, mix=False):
    """Quu + rho I indefinite until the regularisation has grown (negative entries of R, weak terminal weight): the first
    backward passes fail their Cholesky factorisation and restart.  mix: two thirds of the batch start from controls that
    keep them away from the failures (restarts on part of the batch beside instances that finish)."""
    s = make(n, m, N, batch, dtype)
    s.set_model(kind)
    s.set_uniform_step(np.float32(0.05))
    xf = np.tile(0.3 + 0.1 * np.arange(n), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
    R = np.diag([-2e-3 if j % 2 == 0 else 1e-3 for j in range(m)])
    s.set_lqr_cost(0, N, np.eye(n) * 1e-3, R, xf, np.zeros(m))
    s.set_lqr_cost(N, N + 1, np.eye(n) * 0.05, R * 0, xf, np.zeros(m))
    s.set_initial_state(np.zeros(n))
    U = np.full((batch, N, m), 0.05)
    if mix:
        s.add_control_bound(0, N, [-0.1] * m, [0.1] * m)
        U[1::3] = 0.5
        U[2::3] = 0.08
    s.set_trajectory(None, U)
    return s


_kinds = {}


def kind_of(A, n, m):
    """The shape's plugin (a cache hit after build())."""
    if (n, m) not in _kinds:
        os.environ.setdefault("ALTRO_HIP_ARCH", "gfx950")
        src = "#define SHAPE_N %d\n#define SHAPE_M %d\n" % (n, m) + open(os.path.join(ROOT, "tests", "models", "shape_chain.hpp")).read()
        _kinds[(n, m)] = A.register_model_source(f"shape_chain_{n}_{m}", src)
    return _kinds[(n, m)]


_olibs = {}


def oracle_of(A, n, m):
    """Factory of oracle solvers with the shape's model compiled in (oracle/_build/liboracle_shape_<n>_<m>.so)."""
    path = os.path.join(ROOT, "oracle", "_build", f"liboracle_shape_{n}_{m}.so")
    if not os.path.exists(path):
        graft.build_oracle()
    lib = _olibs.setdefault(path, ctypes.CDLL(path))

    def make(n_, m_, N, b, d):
        s = A.BatchSolver(n_, m_, N, b, d, _lib=lib, _prefix="oracle_")
        if b > 64:
            lib.oracle_set_threads(s._h, ctypes.c_int(len(os.sched_getaffinity(0))))
        return s
    return make


def _close(a, b, rtol, atol, label):
    _ledger.close(a, b, rtol, atol, label)


# ---- without a GPU ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_shape_plugin_registers_and_its_oracle_solves(A, n, m):
    """Every shape's plugin compiles (build() leaves it in the cache) -- (1,1) and (2,2) did not before the fix of the 4 x 4
    kernel's gain chunk -- and its oracle solves its own AL problem."""
    assert kind_of(A, n, m) >= A.MODEL_USER_BASE
    o = chain_al(A, oracle_of(A, n, m), A.MODEL_USER_BASE, n, m, batch=24)
    o.solve()
    st = o.get_stats()
    ok = st["status"] == 0
    assert ok.mean() >= 0.9, st["status"]
    X, U = o.get_trajectory()
    assert np.abs(X[ok][:, -1] - chain_goals(n, m, 60, 24)[ok]).max() < 1e-3
    umax = np.abs(U).max(axis=(1, 2))
    assert (umax >= BOUND.get((n, m), 2.0) - 1e-6).any()  # the control bound is active on part of the batch ...
    assert (umax < BOUND.get((n, m), 2.0) - 1e-6).any()  # ... and not on all of it


@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_shape_restart_problem_restarts_on_the_oracle(A, n, m):
    """The restart problem of the GPU tests takes the restart path on the oracle, on every instance."""
    o = chain_restart(A, oracle_of(A, n, m), A.MODEL_USER_BASE, n, m, batch=6)
    o.set_options(max_iterations_inner=4)
    o.solve_ilqr()
    assert (o.get_stats()["regularization"] > 1e-8).all()


# ---- on the GPU: against the oracle --------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_step_level(A, hip_make, n, m):
    """Two sweeps of expansions / backward pass / forward pass in fp64 (the pattern of test_step_level_unicycle): [A|B] and
    lxx ... lu at knots 0, 1, mid, N-1, N; knot costs and constraint values; K, d, P, p; the regularisation and alpha EXACT;
    cost, X and U after the line search."""
    N = 60
    kind = kind_of(A, n, m)
    o = chain_al(A, oracle_of(A, n, m), kind, n, m, batch=8, N=N)
    g = chain_al(A, hip_make, kind, n, m, batch=8, N=N)
    for s in (o, g):
        s.set_record_ctg(True)
        s.rollout()
    _close(g.cost(), o.cost(), 1e-12, 0.0, f"{n}_{m} initial cost")
    _close(g.get_trajectory()[0], o.get_trajectory()[0], 1e-12, 1e-13, f"{n}_{m} X rollout")
    for it in range(2):
        for s in (o, g):
            s.update_expansions()
        for k in (0, 1, N // 2, N - 1, N):
            eo, eg = o.get_expansion(k), g.get_expansion(k)
            for key in ("lxx", "lx") + (("A", "B", "lxu", "luu", "lu") if k < N else ()):
                # (the gradients carry the 2e-10 by which the first line search's U differ into sweep 1: measured 6.1e-11)
                _close(eg[key], eo[key], 1e-10, 1e-9 if key in ("lx", "lu") else 1e-12, f"{n}_{m} expansion {key} (sweep {it})")
        # (measured maxima over the shapes, profiles/r06_parity_errors.json: knot costs 3.2e-10, constraint values 6.1e-11 abs)
        _close(g.get_knot_costs(), o.get_knot_costs(), 1e-11, 3e-9, f"{n}_{m} knot costs (sweep {it})")
        _close(g.get_constraint_values(), o.get_constraint_values(), 1e-10, 6e-10, f"{n}_{m} constraint values (sweep {it})")
        for s in (o, g):
            s.backward_pass()
        assert (o.get_stats()["regularization"] == g.get_stats()["regularization"]).all()
        Ko, do = o.get_gains()
        Kg, dg = g.get_gains()
        Po, po = o.get_ctg()
        Pg, pg = g.get_ctg()
        _ledger.close_normwise(Kg.reshape(-1, m, n), Ko.reshape(-1, m, n), 1e-9, f"{n}_{m} K per knot, normwise (sweep {it})")
        # (measured: K 3.8e-11, P 1.1e-11, p 6.1e-10 norm-wise; d 2.0e-10 abs -- d vanishes where the trajectory is optimal,
        #  so it is held to an absolute bar)
        _close(dg, do, 0.0, 2e-9, f"{n}_{m} d (sweep {it})")
        _ledger.close_normwise(Pg.reshape(-1, n, n), Po.reshape(-1, n, n), 1e-9, f"{n}_{m} P per knot, normwise (sweep {it})")
        _ledger.close_normwise(pg.reshape(-1, n), po.reshape(-1, n), 5e-9, f"{n}_{m} p per knot, normwise (sweep {it})")
        for s in (o, g):
            s.forward_pass()
        so, sg = o.get_stats(), g.get_stats()
        assert (so["alpha"] == sg["alpha"]).all(), (so["alpha"], sg["alpha"])
        _close(sg["cost"], so["cost"], 1e-9, 0.0, f"{n}_{m} cost after the line search (sweep {it})")
        Xo, Uo = o.get_trajectory()
        Xg, Ug = g.get_trajectory()
        _close(Xg, Xo, 1e-8, 1e-10, f"{n}_{m} X after the line search (sweep {it})")
        _close(Ug, Uo, 1e-8, 1e-10, f"{n}_{m} U after the line search (sweep {it})")
        if it == 0:
            assert (sg["alpha"] > 0).any()  # the second sweep starts from a moved trajectory


# Bars of the whole solves, per shape and batch: ~10x the maxima measured on the MI355X (profiles/r06_parity_errors.json),
# never below 1e-14 abs / 1e-13 norm-wise.  (X, U, d, duals: abs; K: norm-wise per instance.)  The chains (7,3), (9,1) and
# (13,2) amplify the rounding of 10 - 20 iterations to 1e-7; (3,1) does too at batch 768, whose long runners iterate 100+
# times; the 4 x 4 shapes (1,1), (1,2), (2,2) agree to the last bits or two.
_AL_BARS = {
    ((1, 1), 40): (1e-14, 5e-14, 2e-13, 2e-12, 5e-14),
    ((1, 1), 768): (1e-14, 1e-13, 2e-13, 2e-12, 5e-14),
    ((1, 2), 40): (1e-14, 1e-13, 5e-13, 2e-12, 5e-14),
    ((1, 2), 768): (1e-14, 1e-13, 5e-13, 5e-12, 5e-14),
    ((2, 2), 40): (1e-14, 1e-13, 1e-12, 1e-13, 5e-13),
    ((2, 2), 768): (1e-14, 2e-13, 1e-12, 1e-12, 5e-13),
    ((3, 1), 40): (1e-13, 2e-12, 2e-12, 2e-12, 5e-12),
    ((3, 1), 768): (2e-07, 1e-06, 1e-10, 5e-08, 2e-07),
    ((3, 5), 40): (2e-13, 2e-12, 5e-10, 1e-12, 5e-12),
    ((5, 3), 40): (5e-12, 5e-11, 5e-09, 2e-09, 1e-11),
    ((6, 5), 40): (5e-11, 2e-10, 5e-08, 5e-09, 2e-11),
    ((7, 3), 40): (1e-06, 1e-05, 2e-06, 5e-07, 1e-05),
    ((9, 1), 40): (2e-06, 1e-05, 5e-12, 5e-12, 2e-05),
    ((13, 2), 40): (5e-07, 5e-06, 5e-07, 1e-07, 1e-05),
}
# ... of the fp32-record solves against the record-rounding oracle (X, U abs; K norm-wise)
_F32_BARS = {
    ((1, 1), 40): (1e-14, 5e-14, 1e-13),
    ((1, 1), 768): (1e-14, 2e-13, 1e-13),
    ((2, 2), 40): (5e-14, 1e-12, 1e-13),
    ((2, 2), 768): (5e-11, 1e-09, 1e-13),
    ((3, 5), 40): (5e-12, 1e-10, 2e-09),
    ((5, 3), 40): (2e-08, 1e-06, 2e-08),
    ((13, 2), 40): (5e-07, 5e-06, 2e-06),
}
# ... and of the MFMA backward kernels against the VALU kernel (abs), per shape, solve and quantity
_MFMA_VALU_BARS = {
    (1, 1): {"al40": (1e-14, 1e-13), "al768": (1e-14, 1e-13), "restart": (1e-14, 1e-13)},
    (1, 2): {"al40": (1e-14, 1e-13), "al768": (1e-14, 1e-13), "restart": (1e-14, 1e-13)},
    (2, 2): {"al40": (1e-14, 1e-13), "al768": (1e-14, 2e-13), "restart": (2e-14, 5e-13)},
    (3, 1): {"al40": (2e-09, 1e-08), "al768": (5e-07, 5e-06), "restart": (2e-14, 2e-13)},
    (5, 3): {"al40": (1e-11, 1e-10), "restart": (5e-14, 5e-13)},
    (7, 3): {"al40": (1e-08, 5e-08), "restart": (5e-14, 5e-13)},
    (9, 1): {"al40": (2e-06, 1e-05), "restart": (1e-13, 5e-13)},
}


def _al_cases():
    cases = []
    for s in SHAPES:
        cases.append((s, 40))
        if s in MFMA4:
            cases.append((s, 768))  # above persist_at_ (2 x the CUs): the device-side sweep loop, then the persistent tail
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("shape,batch", _al_cases(), ids=[f"{n}_{m}-b{b}" for (n, m), b in _al_cases()])
def test_al_solve(A, hip_make, shape, batch):
    """Whole AL solves of jittered goals with a goal constraint and control bounds active on part of the batch: statuses and
    both iteration counts EXACT for every instance; X, U, K, d and the duals within the bars."""
    n, m = shape
    kind = kind_of(A, n, m)
    o = chain_al(A, oracle_of(A, n, m), kind, n, m, batch=batch)
    g = chain_al(A, hip_make, kind, n, m, batch=batch)
    g.set_options(profiler_enable=1)
    o.solve()
    g.solve()
    so, sg = o.get_stats(), g.get_stats()
    tm = g.get_timing()
    print(f"({n},{m}) batch {batch}: iterations up to {so['iterations_total'].max()}, solved {(so['status'] == 0).mean():.3f}, "
          f"sweeps {tm['sweeps']} ({tm['fused_sweeps']} persistent), loop iterations {tm['loop_iterations']}")
    for f in ("status", "iterations_total", "iterations_outer"):
        assert (so[f] == sg[f]).all(), (f, np.flatnonzero(so[f] != sg[f])[:8])
    ok = so["status"] == 0
    assert ok.mean() >= 0.9
    if shape in MFMA4:
        assert tm["fused_sweeps"] > 0  # the persistent kernel took the tail (or the whole small batch)
        if batch > 512:
            assert tm["loop_iterations"] > 0  # ... behind the device-side sweep loop
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    tag = f"{n}_{m} batch {batch}"
    bX, bU, bK, bd, blam = _AL_BARS[(shape, batch)]
    _close(Xg[ok], Xo[ok], 0.0, bX, f"{tag}: X")
    _close(Ug[ok], Uo[ok], 0.0, bU, f"{tag}: U")
    Ko, do = o.get_gains()
    Kg, dg = g.get_gains()
    _ledger.close_normwise(Kg[ok], Ko[ok], bK, f"{tag}: K of the solved instances, normwise")
    _close(dg[ok], do[ok], 0.0, bd, f"{tag}: d of the solved instances")
    _close(g.get_duals()[ok], o.get_duals()[ok], 0.0, blam, f"{tag}: duals")


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_cholesky_restart(A, hip_make, n, m):
    """ilqr.hpp:409-427 (raise the regularisation, restart the sweep) on every shape's backward kernel, against the oracle."""
    kind = kind_of(A, n, m)
    o = chain_restart(A, oracle_of(A, n, m), kind, n, m, batch=6)
    g = chain_restart(A, hip_make, kind, n, m, batch=6)
    for s in (o, g):
        s.set_options(max_iterations_inner=4)
        s.solve_ilqr()
    so, sg = o.get_stats(), g.get_stats()
    assert (so["regularization"] > 1e-8).all()  # the restart path was really taken
    for f in ("status", "iterations_total"):
        assert np.array_equal(sg[f], so[f]), f
    _close(sg["regularization"], so["regularization"], 1e-12, 0.0, f"{n}_{m} regularisation")
    (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
    _close(Xg, Xo, 1e-9, 1e-11, f"{n}_{m} restart X")
    _close(Ug, Uo, 1e-9, 1e-11, f"{n}_{m} restart U")
    _ledger.close_normwise(g.get_gains()[0], o.get_gains()[0], 1e-9, f"{n}_{m} restart K, normwise")


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", F32_SHAPES, ids=ids(F32_SHAPES))
def test_fp32_records(A, hip_make, n, m):
    """fp32 expansion / gain records (WithRec32<>) against the record-rounding oracle (dtype 2): the padding of the fp32
    records differs from the fp64 one for these shapes, so the layouts are new."""
    kind = kind_of(A, n, m)
    for batch in ((40, 768) if (n, m) in MFMA4 else (40,)):
        o = chain_al(A, oracle_of(A, n, m), kind, n, m, batch=batch, dtype=2)
        g = chain_al(A, hip_make, kind, n, m, batch=batch, dtype=A.F32)
        o.solve()
        g.solve()
        so, sg = o.get_stats(), g.get_stats()
        for f in ("status", "iterations_total", "iterations_outer"):
            assert (so[f] == sg[f]).all(), (batch, f, np.flatnonzero(so[f] != sg[f])[:8])
        ok = so["status"] == 0
        assert ok.mean() >= 0.9
        (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
        tag = f"{n}_{m} fp32 records batch {batch}"
        bX, bU, bK = _F32_BARS[((n, m), batch)]
        _close(Xg[ok], Xo[ok], 0.0, bX, f"{tag}: X")
        _close(Ug[ok], Uo[ok], 0.0, bU, f"{tag}: U")
        _ledger.close_normwise(g.get_gains()[0][ok], o.get_gains()[0][ok], bK, f"{tag}: K, normwise")


# Horizons at the boundaries of the gain chunks the backward kernels buffer in LDS: kBwdChunk = 126 knots (4 x 4 kernel),
# kM16Chunk = 32 (16 x 16 kernel).  The 4 x 4 kernel's bulk store walks the chunk's elements (slot x 4 instances x record
# stride) with the lanes of the wavefront; its last pass is partial, and with a 2-element record (1,1) a pass of one knot
# (N = 127, 253) -- or with the 6-element record of (2,2) a pass of three knots (N = 129) -- leaves the lanes of blocks 2 and 3
# idle: the shuffle of their instance index inside that pass returned no value, and their gains of those knots were never
# stored.  Every 4 x 4 shape runs at N = 127; (2,1) is the pendulum plugin, (3,2) the built-in unicycle; fp32 records run
# (1,1) and (2,2) across the chunk too.
_CHUNK_CASES = ([("chain", (1, 1), N, "f64") for N in (126, 127, 129, 253)] +
                [("chain", (2, 2), N, "f64") for N in (125, 126, 127, 129, 253)] +
                [("chain", (1, 2), 127, "f64"), ("chain", (3, 1), 127, "f64"), ("pendulum", (2, 1), 127, "f64"),
                 ("unicycle", (3, 2), 127, "f64")] +
                [("chain", s, N, "f32") for s in ((1, 1), (2, 2)) for N in (126, 127, 253)] +
                [("chain", (5, 3), N, "f64") for N in (31, 32, 33, 65)])


def unicycle_restart_mix(A, make, batch, N, dtype=0):
    """scripts/probe_shapes.py's restart mix on the built-in unicycle."""
    s = make(3, 2, N, batch, dtype)
    s.set_model(A.MODEL_UNICYCLE)
    s.set_uniform_step(np.float32(0.05))
    xf = np.tile(np.array([1.0, 0.5, 0.3]), (batch, 1)) + np.linspace(0, 0.3, batch)[:, None]
    R = np.diag([-2e-3, 1e-3])
    s.set_lqr_cost(0, N, np.eye(3) * 1e-3, R, xf, np.zeros(2))
    s.set_lqr_cost(N, N + 1, np.eye(3) * 10.0, R * 0, xf, np.zeros(2))
    s.add_control_bound(0, N, [-0.1, -0.1], [0.1, 0.1])
    s.set_initial_state(np.zeros(3))
    U = np.zeros((batch, N, 2))
    U[0::3] = 0.05
    U[1::3] = 0.5
    U[2::3] = 0.08
    s.set_trajectory(None, U)
    return s


def _chunk_problem(A, model, shape, N, batch, make, dtype):
    n, m = shape
    if model == "unicycle":
        return unicycle_restart_mix(A, make, batch, N, dtype)
    if model == "pendulum":
        kind = A.register_model_source("pendulum", open(os.path.join(ROOT, "tests", "models", "pendulum.hpp")).read())
    else:
        kind = kind_of(A, n, m)
    return chain_restart(A, make, kind, n, m, batch=batch, N=N, mix=True, dtype=dtype)


def _chunk_oracle(A, model, shape, oracle_make):
    if model == "unicycle":
        return oracle_make
    if model == "pendulum":
        path = os.path.join(ROOT, "oracle", "_build", "liboracle_pendulum.so")
        if not os.path.exists(path):
            graft.build_oracle()
        lib = _olibs.setdefault(path, ctypes.CDLL(path))

        def make(n_, m_, N, b, d):
            s = A.BatchSolver(n_, m_, N, b, d, _lib=lib, _prefix="oracle_")
            lib.oracle_set_threads(s._h, ctypes.c_int(len(os.sched_getaffinity(0))))
            return s
        return make
    return oracle_of(A, *shape)


@pytest.mark.gpu
@pytest.mark.parametrize("model,shape,N,rec", _CHUNK_CASES,
                         ids=[f"{mo}_{n}_{m}-N{N}-{r}" for mo, (n, m), N, r in _CHUNK_CASES])
def test_gain_chunk_horizons(A, hip_make, oracle_make, model, shape, N, rec):
    """Restarts beside instances that pass their factorisation in the same backward pass (the reduced restart mix of the
    N > 126 bulk-store bug: a third of the batch starts outside the control bounds, whose penalty makes Quu definite),
    at horizons around the gain chunks; small and large batch (persistent kernel / device loop and batched sweeps); fp64
    against the fp64 oracle, fp32 records against the record-rounding oracle.  Schedules exact; X, K and d to 1e-9."""
    n, m = shape
    omake = _chunk_oracle(A, model, shape, oracle_make)
    for batch in (7, 640):
        o = _chunk_problem(A, model, shape, N, batch, omake, 0 if rec == "f64" else 2)
        g = _chunk_problem(A, model, shape, N, batch, hip_make, A.F64 if rec == "f64" else A.F32)
        for s in (o, g):
            s.set_options(max_iterations_inner=3, max_iterations_outer=1)
            s.solve()
        so, sg = o.get_stats(), g.get_stats()
        assert (so["regularization"] > 1e-8).any()  # the restart path was taken
        for f in ("status", "iterations_total"):
            assert np.array_equal(sg[f], so[f]), (batch, f, np.flatnonzero(sg[f] != so[f])[:8])
        tag = f"{model} {n}_{m} N {N} {rec} batch {batch}"
        (Xo, Uo), (Xg, Ug) = o.get_trajectory(), g.get_trajectory()
        (Ko, do), (Kg, dg) = o.get_gains(), g.get_gains()
        # (measured on the chains: X 6e-15, K 6e-15 abs; the unicycle's restart mix is the probe that found round 6's
        #  bulk-store bug)
        _close(Xg, Xo, 1e-9, 1e-11, f"{tag}: restart mix X")
        _ledger.close_normwise(Kg, Ko, 1e-9, f"{tag}: restart mix K, normwise")
        _close(dg, do, 1e-9, 1e-11, f"{tag}: restart mix d")


# ---- on the GPU: the kernels against each other (child processes) --------------------------------------------------------

_CHILD = r'''
import os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import test_model_shapes_gpu as T
A = T.graft.load_package()
make = lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)
out = {}
def dump(tag, s):
    st = s.get_stats()
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    out[tag + "_X"], out[tag + "_U"], out[tag + "_K"], out[tag + "_d"], out[tag + "_lam"] = X, U, K, d, s.get_duals()
    for f in ("status", "iterations_total", "iterations_outer", "cost", "regularization"):
        out[tag + "_" + f] = st[f]
for n, m in T.SHAPES:
    kind = T.kind_of(A, n, m)
    for batch in ((40, 768) if (n, m) in T.MFMA4 else (40,)):
        s = T.chain_al(A, make, kind, n, m, batch=batch); s.solve(); dump(f"{n}_{m}_al{batch}", s)
    s = T.chain_restart(A, make, kind, n, m, batch=6); s.set_options(max_iterations_inner=4); s.solve_ilqr()
    dump(f"{n}_{m}_restart", s)
np.savez(sys.argv[1], **out)
'''

_VARIANTS = {"default": {}, "valu": {"ALTRO_HIP_BACKWARD": "valu"}, "coop": {"ALTRO_HIP_BACKWARD": "coop"},
             "batched": {"ALTRO_HIP_NO_FUSED_SWEEP": "1"}, "sweeps": {"ALTRO_HIP_SWEEP_LOOP": "0"},
             "fwd_lds": {"ALTRO_HIP_FWD_SRC": "lds"}, "fwd_global": {"ALTRO_HIP_FWD_SRC": "global"}}


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    d = tmp_path_factory.mktemp("shapes")
    res = {}
    for tag, env in _VARIANTS.items():
        out = str(d / f"{tag}.npz")
        subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}, out], check=True, env=dict(os.environ, **env), timeout=900)
        res[tag] = np.load(out)
    return res


def _keys(v, n, m):
    return [k for k in v.files if k.startswith(f"{n}_{m}_")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", COOP, ids=ids(COOP))
def test_coop_backward_is_bitwise_the_valu_backward(variants, n, m):
    """k_backward_coop performs riccati_q / riccati_gains' operations in the same order and type (its header): the default
    kernel of these shapes returns the bits of the VALU kernel."""
    for k in _keys(variants["default"], n, m):
        assert np.array_equal(variants["default"][k], variants["valu"][k]), k
        assert np.array_equal(variants["coop"][k], variants["valu"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", MFMA4 + MFMA16, ids=ids(MFMA4 + MFMA16))
def test_mfma_backward_agrees_with_valu(variants, n, m):
    """The matrix-core kernels associate the products differently from the VALU kernel: same schedule (statuses, iteration
    counts, regularisation), values to rounding."""
    a, b = variants["default"], variants["valu"]
    for k in _keys(a, n, m):
        if k.endswith(("_status", "_iterations_total", "_iterations_outer", "_regularization")):
            assert np.array_equal(a[k], b[k]), k
        elif k.endswith(("_X", "_U")):
            solve = k.split("_")[2]  # al40 / al768 / restart
            bX, bU = _MFMA_VALU_BARS[(n, m)][solve]
            _close(a[k], b[k], 0.0, bX if k.endswith("_X") else bU, f"{n}_{m} MFMA vs VALU {k.split('_', 2)[2]}")


# Open finding: at (3,1) the persistent kernel's results differ from the batched sweeps' in the last bits (X 1e-14, K 8e-12
# abs, same schedule), deterministically and from a batch of one on; (1,1), (2,2), (1,2), the pendulum (2,1) and the
# unicycle (3,2) are bitwise.  The device-side loop and the host-paced sweeps hand their instances to the persistent kernel
# at different iterations, so at batch 768 the difference shows between those two as well (their batch-40 solves, persistent
# kernel only, agree).  Strict: a change either way is reported.
_OPEN_3_1 = pytest.mark.xfail(reason="(3,1): k_sweep_fused and the batched sweeps differ in the last bits; cause not found",
                              strict=True)


def _mfma4_params():
    return [pytest.param(n, m, id=f"{n}_{m}", marks=[_OPEN_3_1] if (n, m) == (3, 1) else []) for n, m in MFMA4]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", _mfma4_params())
def test_loop_is_bitwise_the_sweeps(variants, n, m):
    """4 x 4 shapes: the device-side sweep loop (k_sweep_loop, default above the hand-over) == the host-paced sweeps
    (ALTRO_HIP_SWEEP_LOOP=0), bit for bit."""
    for k in _keys(variants["default"], n, m):
        assert np.array_equal(variants["default"][k], variants["sweeps"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", _mfma4_params())
def test_persistent_is_bitwise_the_batched_sweeps(variants, n, m):
    """4 x 4 shapes: the persistent kernel (k_sweep_fused, the tail of the host-paced sweeps) == the batched sweeps alone
    (ALTRO_HIP_NO_FUSED_SWEEP=1), bit for bit."""
    for k in _keys(variants["sweeps"], n, m):
        assert np.array_equal(variants["sweeps"][k], variants["batched"][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_forward_sources_are_bitwise_equal(variants, n, m):
    """The forward pass's sources of its per-knot inputs (ALTRO_HIP_FWD_SRC = lds | global, and the default choice --
    kSrcKdg where the shape is eligible) return the same bits."""
    for other in ("fwd_lds", "fwd_global"):
        for k in _keys(variants["default"], n, m):
            assert np.array_equal(variants["default"][k], variants[other][k]), (other, k)
