"""altro_lqr_gains and altro_cov_propagate on the ten shapes (n, m) of tests/models/shape_chain.hpp, against their numpy
statements (tests/_lqr_common.py, tests/_cov_common.py).

k_lqr_recur and k_cov_recur spread an instance over a group of G = 2^ceil(log2 n) lanes; the built-in models and the cart-pole
reach G = 4, 8, 16 with one or two dead lanes and m = 1, 2, 4.  The shapes here add G = 1 (64 instances per wave, a one-bit
ballot mask), G = 2, groups with 3 of 8, 7 and 3 of 16 dead lanes, m = 3 and m = 5 (packed S of 6 and 15 entries), m > n
((1, 2), (3, 5)) and the gain records of (1, 1) and (2, 2), which pad to 2 / 4 and 6 / 8 elements in fp32 / fp64.

One case per shape, built once: N = 24, B = 67 (every group size gets more than one workgroup of the recursions and a last one
holding 3 instances), a plan per instance (tests/_recur_common.py: plan) rolled out on the device -- no solve -- and A_k, B_k
from the shape's own oracle at that trajectory, as tests/test_lqr_gpu.py takes them.  The bars are those of
tests/test_lqr_gpu.py and tests/test_cov_gpu.py, through the same functions."""
import numpy as np
import pytest

import _cov_common as CC
import _lqr_common as LC
import _recur_common as RC
import _subset_common as SC
from test_cov_gpu import _check as cov_check
from test_cov_gpu import _handle_state, _inputs, _same_state
from test_model_shapes_gpu import F32_SHAPES, SHAPES, chain_goals, ids, kind_of, oracle_of

pytestmark = pytest.mark.gpu

N, B = RC.N, 67


def _handle(A, make, n, m, batch, dtype=0):
    """the LQR cost of chain_al without its constraints, the step, no plan yet"""
    s = make(n, m, N, batch, dtype)
    hd = float(np.float32(0.05))
    xf = chain_goals(n, m, N, batch)
    s.set_model(kind_of(A, n, m))
    s.set_uniform_step(np.float32(0.05))
    s.set_lqr_cost(0, N, np.eye(n) * (0.1 * hd), np.eye(m) * (1e-2 * hd), xf, np.zeros(m))
    s.set_lqr_cost(N, N + 1, np.eye(n) * 10.0, np.zeros((m, m)), xf, np.zeros(m))
    return s


def _with_plan(A, make, n, m, X, U, dtype=0):
    """a handle that holds the trajectory X [b][N + 1][n], U [b][N][m]"""
    s = _handle(A, make, n, m, X.shape[0], dtype)
    s.set_initial_state(X[:, 0])
    s.set_trajectory(X, U)
    return s


_CASES = {}


def case(A, hip_make, n, m):
    """-> dict(g: the GPU handle with the rolled-out plan, X, U: that trajectory, A, B: the oracle's Jacobians there
    [B][N][n][.], ref: the statement at LC.parity_weights, installed: whether g holds the LQR gains yet)"""
    if (n, m) not in _CASES:
        x0, u = RC.plan(n, m, B)
        g = _handle(A, hip_make, n, m, B)
        g.set_initial_state(x0)
        g.set_trajectory(None, np.repeat(u[:, None, :], N, axis=1))
        g.rollout()
        X, U = g.get_trajectory()
        o = _handle(A, oracle_of(A, n, m), n, m, B)
        o.set_initial_state(x0)
        o.set_trajectory(X, U)
        o.update_expansions()
        ex = [o.get_expansion(k) for k in range(N)]
        o.close()
        c = dict(g=g, X=X, U=U, A=np.stack([e["A"] for e in ex], axis=1), B=np.stack([e["B"] for e in ex], axis=1), installed=False)
        c["ref"] = LC.reference(c["A"], c["B"], *LC.parity_weights(n, m))
        _CASES[(n, m)] = c
    return _CASES[(n, m)]


def _installed(c, n, m):
    """the case's handle with the LQR gains of LC.parity_weights installed (once); -> K as the handle holds it"""
    if not c["installed"]:
        got = c["g"].lqr_gains(*LC.parity_weights(n, m), install=True, want=("fail",))
        assert (got["fail"] == -1).all()
        c["installed"] = True
    return c["g"].get_gains()[0].copy()


# ---- a. parity with the numpy statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_lqr_parity(A, hip_make, n, m):
    c = case(A, hip_make, n, m)
    Q, R, Qf = LC.parity_weights(n, m)
    got = c["g"].lqr_gains(Q, R, Qf)
    fr = {}
    try:
        LC.parity(f"lqr_gains {n}_{m}", c["ref"], got, N, n, m, fr)
    finally:
        RC.record(f"lqr_gains {n}_{m}", fr[f"lqr_gains {n}_{m}"])
    assert (got["P"] == np.swapaxes(got["P"], 2, 3)).all()
    assert (got["P"][:, N] == CC.lower_sym(Qf)).all()


# ---- b. the failure path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_lqr_failure_path(A, hip_make, n, m):
    """Qf = diag(1, .., 1, 50, -v) cut to its last n entries, v chosen with the statement so that a quarter to three quarters of
    the instances fail and no pivot sits on the edge.  At G = 1 and G = 2 failing and surviving instances are neighbouring
    lanes of one wave: the only test of the ballot's group mask there."""
    c = case(A, hip_make, n, m)
    Q, R, Qf0 = LC.parity_weights(n, m)
    Qf, K, Pm, fail = RC.mixed_failure(c["A"], c["B"], Q, R, n, f"{n}_{m}")
    RC.check_failure(c["g"].lqr_gains(Q, R, Qf), K, Pm, fail)
    # install: first gains nobody fails on, then the mixed call: the failed instances keep the first, the others get theirs
    s = _with_plan(A, hip_make, n, m, c["X"], c["U"])
    assert (s.lqr_gains(Q, R, Qf0, install=True, want=("fail",))["fail"] == -1).all()
    before = SC.snapshot(s)
    inst = s.lqr_gains(Q, R, Qf, install=True)
    after = SC.snapshot(s)
    bad = inst["fail"] >= 0
    assert (inst["fail"] == fail).all() and bad.any() and (~bad).any()
    assert not SC.differing(after, before, bad), SC.differing(after, before, bad)
    changed = SC.differing(after, before, ~bad)
    assert "K" in changed and set(changed) <= {"K", "d"}, changed
    assert np.ascontiguousarray(after["K"][~bad]).tobytes() == np.ascontiguousarray(inst["K"][~bad]).tobytes()
    assert (after["d"] == 0).all()
    s.close()


# ---- c. install: the gain record of every padding ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["F64", "F32"])
@pytest.mark.parametrize("n,m", F32_SHAPES, ids=ids(F32_SHAPES))
def test_lqr_install(A, hip_make, n, m, dtype_name):
    """batch 5; (1, 1) and (2, 2) are the shapes whose record K | d pads to 2 / 4 and 6 / 8 elements in fp32 / fp64"""
    c = case(A, hip_make, n, m)
    s = _handle(A, hip_make, n, m, 5, getattr(A, dtype_name))
    s.set_initial_state(c["X"][:5, 0])
    s.set_trajectory(None, c["U"][:5])
    s.rollout()
    Q, R, Qf = LC.parity_weights(n, m)
    before = _handle_state(s)
    got = s.lqr_gains(Q, R, Qf, install=False)
    _same_state(before, _handle_state(s), "install = 0")
    inst = s.lqr_gains(Q, R, Qf, install=True)
    for k in got:
        assert got[k].tobytes() == inst[k].tobytes(), k
    assert (got["fail"] == -1).all() and np.isfinite(got["K"]).all() and np.abs(got["K"]).max() > 0
    after = _handle_state(s)
    want = got["K"].astype(np.float32).astype(np.float64) if dtype_name == "F32" else got["K"]
    Kh, dh = s.get_gains()
    assert np.ascontiguousarray(Kh).tobytes() == np.ascontiguousarray(want).tobytes()
    assert (dh == 0).all() and not np.signbit(dh).any()
    for k in before:
        if k not in ("K", "d"):
            assert before[k].tobytes() == after[k].tobytes(), k
    with pytest.raises(A.AltroError) as e:
        s.get_ctg()
    assert f"({A.NOT_READY})" in str(e.value)
    assert _handle_state(s)["K"].tobytes() == after["K"].tobytes()
    s.close()


# ---- d. the covariance under the installed gains ----------------------------------------------------------------------------------------
def _cov_forms(n, seed):
    """(tag, Sigma0, W, w_mode) of the two forms: W per instance and knot with Sigma0 per instance; one W with one Sigma0"""
    Sigma0, W = _inputs(B, n, N, seed)
    return (("w_mode 3, Sigma0 per instance", Sigma0, W, 3), ("w_mode 0, Sigma0 shared", Sigma0[0], W[0, 0], 0))


@pytest.mark.parametrize("n,m", SHAPES, ids=ids(SHAPES))
def test_cov_parity(A, hip_make, n, m):
    c = case(A, hip_make, n, m)
    g = c["g"]
    K = _installed(c, n, m)  # (the gains are an input of the statement)
    want = ("Sigma", "sx", "su", "rpos") if n >= 2 else ("Sigma", "sx", "su")
    for tag, Sigma0, W, w_mode in _cov_forms(n, 100 + 10 * n + m):
        got = g.cov_propagate(N, Sigma0, W, want=want)
        fr = cov_check(f"{n}_{m} {tag}", got, dict(A=c["A"], B=c["B"], K=K), N, Sigma0, W, w_mode, N, n)
        RC.record(f"cov_propagate {n}_{m}", fr)
        assert (got["Sigma"] == np.swapaxes(got["Sigma"], 2, 3)).all()
    if n < 2:  # the position spread reads two states
        with pytest.raises(A.AltroError) as e:
            g.cov_propagate(N, Sigma0, W, want=("rpos",))
        assert f"({A.INVALID_ARG})" in str(e.value)


# ---- e. an instance alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", [(1, 2), (2, 2), (13, 2)], ids=ids([(1, 2), (2, 2), (13, 2)]))
def test_independent_of_the_neighbours(A, hip_make, n, m):
    """the plans of instances 0, 37 and 66 alone on handles of batch 1: the bits they have inside the batch of 67"""
    c = case(A, hip_make, n, m)
    g = c["g"]
    Q, R, Qf = LC.parity_weights(n, m)
    _installed(c, n, m)
    got = g.lqr_gains(Q, R, Qf)
    _, Sigma0, W, _ = _cov_forms(n, 7)[0]
    want = ("Sigma", "sx", "su", "rpos") if n >= 2 else ("Sigma", "sx", "su")
    cov = g.cov_propagate(N, Sigma0, W, want=want)
    for b in (0, 37, 66):
        one = _with_plan(A, hip_make, n, m, c["X"][b:b + 1], c["U"][b:b + 1])
        alone = one.lqr_gains(Q, R, Qf, install=True)
        for k in ("K", "P", "fail"):
            assert alone[k][0].tobytes() == got[k][b].tobytes(), (b, k)
        cov1 = one.cov_propagate(N, Sigma0[b:b + 1], W[b:b + 1], want=want)
        for k in want:
            assert cov1[k][0].tobytes() == cov[k][b].tobytes(), (b, k)
        one.close()
