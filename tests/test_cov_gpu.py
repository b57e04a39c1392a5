"""Closed-loop covariance on the device (include/altro_covariance.h) against its numpy statement (tests/_cov_common.py).

The inputs of the statement: A_k, B_k from the CPU oracle, which is given the GPU's trajectory (set_trajectory,
update_expansions, get_expansion), and K from the GPU's get_gains -- the gains are an input of the computation, not its
result.  The error of a matrix is max |gpu - numpy| / max |numpy| per (instance, knot); its bar is the larger of
  * 8 x the same quantity between the float64 and the np.longdouble run of the statement on the same inputs (the reference's
    own rounding sensitivity; the factor 8 because the summation order and the FMA contraction of the kernel are free), and
  * 4 N n 2^-52, the length of the accumulation, which takes over where the longdouble difference is zero.
Every handle and every reference is built once and shared by the tests (nothing here changes a handle but test 9's own)."""
import numpy as np
import pytest

import _cov_common as CC
from test_knot_shapes_gpu import TIGHT, _against_the_oracle
from test_mpc_track_gpu import DeviceBuffer

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


# ---- the cases: (GPU handle, oracle handle) solved / linearised once -----------------------------------------------------------
def _x0s(B, x0):
    """a different initial state per instance: x0 + 0.05 (b + 1) on the first two states, -0.03 b on the third"""
    x = np.tile(np.asarray(x0, dtype=np.float64), (B, 1))
    x[:, 0] += 0.05 * (np.arange(B) + 1)
    x[:, 1] -= 0.02 * np.arange(B)
    x[:, 2] -= 0.03 * np.arange(B)
    return x


def _build(A, P, make, name):
    if name in ("turn90", "turn90_f32", "turn90_67", "turn90_steps", "turn90_2"):
        N, B = {"turn90": (8, 3), "turn90_f32": (8, 3), "turn90_67": (3, 67), "turn90_steps": (5, 2), "turn90_2": (8, 2)}[name]
        s = P.unicycle_turn90(make, batch=B, N=N, dtype=A.F32 if name == "turn90_f32" else A.F64)
        if name == "turn90_steps":  # the general path: per-knot steps and times
            steps = (0.6 * (1.0 + 0.1 * np.sin(1.0 + np.arange(N)))).astype(np.float32)
            s.set_steps(steps)
            s.set_times(np.concatenate([[0.0], np.cumsum(steps)]).astype(np.float32))
        s.set_initial_state(_x0s(B, np.zeros(3)))
        return s, "solve"
    if name == "tripleint":
        s = P.triple_integrator(make, batch=2, N=6, constraints=True)
        s.set_initial_state(_x0s(2, -np.array([1.0, 2.0, 0, 0, 0, 0])))
        return s, "solve"
    assert name == "quad12"
    s = P.quadrotor12(make, batch=2, N=5, dtype=A.F64)
    s.set_initial_state(_x0s(2, np.zeros(12)))
    s.set_options(max_iterations_total=3, max_iterations_inner=3)
    return s, "solve_ilqr"


_CASES = {}


def case(A, P, hip_make, oracle_make, name):
    """-> dict(g: the solved GPU handle, A, B: the oracle's Jacobians at the GPU's trajectory [B][N][n][.], K: the GPU's gains)"""
    if name not in _CASES:
        g, how = _build(A, P, hip_make, name)
        getattr(g, how)()
        X, U = g.get_trajectory()
        o, _ = _build(A, P, oracle_make, "turn90" if name == "turn90_f32" else name)  # (Jacobians in fp64 on both sides)
        o.set_trajectory(X, U)
        o.update_expansions()
        ex = [o.get_expansion(k) for k in range(g.N)]
        o.close()
        _CASES[name] = dict(g=g, A=np.stack([e["A"] for e in ex], axis=1), B=np.stack([e["B"] for e in ex], axis=1),
                            K=g.get_gains()[0].copy())
    return _CASES[name]


def _inputs(B, n, steps, seed):
    """PSD Sigma0 [B][n][n] and W [B][steps][n][n], made unsymmetric above the diagonal (never read)"""
    rng = np.random.RandomState(seed)
    G = 0.05 * rng.randn(B, n, n)
    H = 0.01 * rng.randn(B, steps, n, n)
    junk = np.triu(np.ones((n, n)), 1) * 3.0
    return G @ np.swapaxes(G, 1, 2) + 1e-4 * np.eye(n) + junk, H @ np.swapaxes(H, 2, 3) + 1e-6 * np.eye(n) - junk


_W_SHAPES = ((0, lambda W: W[0, 0]), (CC.W_PER_INSTANCE, lambda W: W[:, 0]), (CC.W_PER_KNOT, lambda W: W[0]), (3, lambda W: W))


def _check(tag, got, c, steps, Sigma0, W, w_mode, N, n):
    """Sigma, sx, su and rpos of one call against the statement, every (instance, knot) against its own reference"""
    ref, refL = {}, {}
    for dst, dtype in ((ref, np.float64), (refL, np.longdouble)):
        dst["Sigma"] = CC.propagate(c["A"], c["B"], c["K"], steps, Sigma0, W, w_mode, dtype=dtype)
        dst["sx"], dst["su"], dst["rpos"] = CC.spreads(dst["Sigma"], c["K"], dtype=dtype)
    floor = 4 * N * n * EPS
    worst = {}
    missed = []
    for name in ("Sigma", "sx", "su", "rpos"):
        if name not in got:
            continue
        # as matrices: Sigma [..][n][n] as it is, sx / su [..][1][len], rpos [..][1][1]
        mat = {"Sigma": lambda a: a, "sx": lambda a: a[..., None, :], "su": lambda a: a[..., None, :], "rpos": lambda a: a[..., None, None]}[name]
        g, r, rl = mat(got[name]), mat(ref[name]), mat(refL[name])
        assert g.shape == r.shape, (tag, name, g.shape, r.shape)
        # the statement against itself in longdouble (the difference taken in longdouble)
        own = (np.abs(r.astype(np.longdouble) - rl).max(axis=(-1, -2))
               / np.maximum(np.abs(rl).max(axis=(-1, -2)), np.longdouble(1e-300))).astype(np.float64)
        bar = np.maximum(8.0 * own, floor)
        scale = np.abs(r).max(axis=(-1, -2))
        err = CC.matrix_rel(g, r)
        worst[name] = (float(err.max()), float((err / bar).max()))
        for idx in np.ndindex(*scale.shape):
            if not np.allclose(g[idx], r[idx], rtol=0, atol=bar[idx] * scale[idx]):
                missed.append((name, idx, float(err[idx]), float(bar[idx])))
    print(f"{tag}: " + ", ".join(f"{k} err {v[0]:.2e} ({v[1]:.2f} of its bar)" for k, v in worst.items()))
    assert not missed, (tag, missed[:6])
    return {k: v[1] for k, v in worst.items()}  # (the largest error of each array as a fraction of its bar)


def _parity(A, P, hip_make, oracle_make, name, seed):
    c = case(A, P, hip_make, oracle_make, name)
    g = c["g"]
    B, N, n = g.batch, g.N, g.n
    Sigma0, W = _inputs(B, n, N, seed)
    for w_mode, pick in _W_SHAPES:
        for S0 in (Sigma0, Sigma0[0]):
            got = g.cov_propagate(N, S0, pick(W))
            _check(f"{name} w_mode {w_mode} Sigma0 {'per instance' if S0.ndim == 3 else 'shared'}", got, c, N, S0, pick(W), w_mode, N, n)
    return c


# ---- 1. parity with the numpy statement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turn90", "tripleint", "quad12"])
def test_parity(A, P, hip_make, oracle_make, name):
    """unicycle_turn90 N = 8 batch 3 after solve_al; triple integrator (n = 6) N = 6 batch 2; quad12 N = 5 batch 2 after
    solve_ilqr capped at 3 iterations; all four w_mode shapes, shared and per-instance Sigma0."""
    _parity(A, P, hip_make, oracle_make, name, seed=11)


# ---- 2. wave boundaries ------------------------------------------------------------------------------------------------------------
def test_wave_boundaries(A, P, hip_make, oracle_make):
    """batch 67 (16 instances per workgroup of k_cov_recur, 64 per workgroup of k_cov_linearise): every instance against its own
    reference, so an indexing slip across lanes or lane groups shows."""
    _parity(A, P, hip_make, oracle_make, "turn90_67", seed=12)


# ---- 3. steps < N ------------------------------------------------------------------------------------------------------------------
def test_fewer_steps_than_knots(A, P, hip_make, oracle_make):
    c = case(A, P, hip_make, oracle_make, "turn90")
    g = c["g"]
    B, N, n, m, steps = g.batch, g.N, g.n, g.m, 3
    Sigma0, W = _inputs(B, n, N, 13)
    W = W[:, :steps]
    got = g.cov_propagate(steps, Sigma0, W)
    assert got["Sigma"].shape == (B, steps + 1, n, n) and got["sx"].shape == (B, steps + 1, n)
    assert got["su"].shape == (B, steps, m) and got["rpos"].shape == (B, steps + 1)
    _check("steps 3 of 8", got, c, steps, Sigma0, W, 3, N, n)
    # canaries behind the rows in over-allocated device buffers
    sizes = dict(Sigma=B * (steps + 1) * n * n, sx=B * (steps + 1) * n, su=B * steps * m, rpos=B * (steps + 1))
    pad = 64
    d0, dW = DeviceBuffer(Sigma0.nbytes, Sigma0), DeviceBuffer(W.nbytes, np.ascontiguousarray(W))
    bufs = {k: DeviceBuffer(8 * (v + pad), np.full(v + pad, -77.0)) for k, v in sizes.items()}
    g.cov_propagate_device(steps, d0.ptr, True, dW.ptr, 3, bufs["Sigma"].ptr, bufs["sx"].ptr, bufs["su"].ptr, bufs["rpos"].ptr)
    for k, v in sizes.items():
        out = bufs[k].read(np.float64, (v + pad,))
        assert out[:v].tobytes() == got[k].tobytes(), k
        assert (out[v:] == -77.0).all(), k
    # rpos alone
    alone = g.cov_propagate(steps, Sigma0, W, want=("rpos",))
    assert list(alone) == ["rpos"] and alone["rpos"].tobytes() == got["rpos"].tobytes()
    for b in list(bufs.values()) + [d0, dW]:
        b.free()


# ---- 4. the general path: per-knot steps and times ---------------------------------------------------------------------------------
def test_per_knot_steps_and_times(A, P, hip_make, oracle_make):
    _parity(A, P, hip_make, oracle_make, "turn90_steps", seed=14)


# ---- 5. an ALTRO_F32 handle ----------------------------------------------------------------------------------------------------------
def test_f32_handle(A, P, hip_make, oracle_make):
    """K is the widened fp32 record on both sides (get_gains returns it), the Jacobians are fp64: the same bar."""
    c = _parity(A, P, hip_make, oracle_make, "turn90_f32", seed=15)
    assert (c["K"] == c["K"].astype(np.float32)).all()


# ---- 6. exact properties -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["turn90", "tripleint", "quad12"])
def test_exact_properties(A, P, hip_make, oracle_make, name):
    g = case(A, P, hip_make, oracle_make, name)["g"]
    B, N, n, m = g.batch, g.N, g.n, g.m
    Sigma0, W = _inputs(B, n, N, 16)
    got = g.cov_propagate(N, Sigma0, W)
    assert (got["Sigma"] == np.swapaxes(got["Sigma"], 2, 3)).all() and np.isfinite(got["Sigma"]).all()
    assert np.abs(got["Sigma"]).max() > 0
    again = g.cov_propagate(N, Sigma0, W)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    zero = g.cov_propagate(N, np.zeros((n, n)), None)
    for k in zero:
        assert (zero[k] == 0).all(), k
    none = g.cov_propagate(N)
    for k in none:
        assert (none[k] == 0).all(), k
    # the device variant: every array in device memory
    d0, dW = DeviceBuffer(Sigma0.nbytes, Sigma0), DeviceBuffer(W.nbytes, W)
    bufs = {k: DeviceBuffer(v.nbytes, np.full(v.shape, -1.0)) for k, v in got.items()}
    g.cov_propagate_device(N, d0.ptr, True, dW.ptr, 3, bufs["Sigma"].ptr, bufs["sx"].ptr, bufs["su"].ptr, bufs["rpos"].ptr)
    for k, v in got.items():
        assert bufs[k].read(np.float64, v.shape).tobytes() == v.tobytes(), k
    for b in list(bufs.values()) + [d0, dW]:
        b.free()


# ---- 7. the handle is untouched ------------------------------------------------------------------------------------------------------
def _handle_state(s):
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    e0 = s.get_expansion(0)
    out = dict(X=X, U=U, K=K.copy(), d=d, lam=s.get_duals(), rho=s.get_penalties(), cval=s.get_constraint_values(), stats=s.get_stats())
    out.update({"exp_" + k: np.ascontiguousarray(v) for k, v in e0.items()})
    return out


def _same_state(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def test_propagation_leaves_the_handle(A, P, hip_make, oracle_make):
    g = case(A, P, hip_make, oracle_make, "turn90")["g"]
    before = _handle_state(g)
    Sigma0, W = _inputs(g.batch, g.n, g.N, 17)
    g.cov_propagate(g.N, Sigma0, W)
    g.cov_propagate(3, Sigma0[0], None, want=("su",))
    _same_state(before, _handle_state(g), "cov_propagate")


# ---- 8. agreement with altro_mpc_track -------------------------------------------------------------------------------------------------
def test_agrees_with_mpc_track(A, P, hip_make, oracle_make):
    """dx0 = +-eps e_i (2 n samples), no disturbance, no clipping: d_i,k = (x+_k - x-_k) / 2 and sum_i d_i d_i^T against
    cov_propagate from Sigma0 = eps^2 I without W.  The truncation error is second order in eps: from 1e-3 to 5e-4 the
    matrix-wise relative error must fall by a factor of at least 3 (ideal: 4).  No absolute number is fixed."""
    g = case(A, P, hip_make, oracle_make, "turn90_2")["g"]
    B, N, n = g.batch, g.N, g.n
    errs = []
    for eps in (1e-3, 5e-4):
        dx0 = np.zeros((B, 2 * n, n))
        for i in range(n):
            dx0[:, 2 * i, i], dx0[:, 2 * i + 1, i] = eps, -eps
        X = g.mpc_track(N, 2 * n, dx0=dx0)["X_cl"]
        d = (X[:, 0::2] - X[:, 1::2]) / 2  # [B][n][N + 1][n]
        sampled = np.einsum("bika,bikc->bkac", d, d)
        Sigma = g.cov_propagate(N, eps * eps * np.eye(n), None, want=("Sigma",))["Sigma"]
        errs.append(CC.matrix_rel(sampled, Sigma)[:, 1:].max())
    print(f"sampled against propagated covariance: relative error {errs[0]:.3e} at eps 1e-3, {errs[1]:.3e} at 5e-4, ratio {errs[0] / errs[1]:.2f}")
    assert errs[1] > 0 and errs[0] / errs[1] >= 3.0


# ---- 9. inflation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("per_instance", [False, True])
def test_inflation(A, P, hip_make, oracle_make, per_instance, offset):
    """A unicycle with one knot circle constraint on [1, N) (tests/_cov_common.py: circle_problem), N = 12, batch 3, a base
    track of 8 rows (fewer than the window: the held end applies).  The inflated parameters against the statement; a second
    call gives the same bits; the handle is untouched but for the track; then solve_al on the inflated track against the
    oracle given the same per-knot radii (tests/test_knot_shapes_gpu.py: _against_the_oracle at TIGHT)."""
    N, B = CC.CIRCLE_N, CC.CIRCLE_B
    base = CC.circle_base(B if per_instance else 0)
    g = CC.circle_problem(A, P, hip_make, base, offset)
    g.solve()
    rpos = g.cov_propagate(N, CC.CIRCLE_SIGMA0, CC.CIRCLE_W, want=("rpos",))["rpos"]
    before = _handle_state(g)
    g.cov_inflate_circles(g.knot_circle, base, CC.CIRCLE_KAPPA, rpos)
    assert g.get_track_offset() == offset
    _same_state(before, _handle_state(g), "cov_inflate_circles")
    par = g.get_knot_params(g.knot_circle)  # [B][N - 1][3]: knots 1 .. N - 1
    track = CC.inflate(base, B, CC.CIRCLE_KAPPA, rpos, offset, N)
    want = track[:, np.minimum(offset + np.arange(1, N), track.shape[1] - 1)]
    src = np.broadcast_to(base, (B,) + base.shape[-2:])[:, np.minimum(offset + np.arange(1, N), base.shape[-2] - 1)]
    assert par[:, :, :2].tobytes() == np.ascontiguousarray(src[:, :, :2]).tobytes()
    assert (np.abs(par[:, :, 2] - want[:, :, 2]) <= 2 * np.spacing(want[:, :, 2])).all()
    assert (par[:, :, 2] > src[:, :, 2]).all()  # (it did inflate)
    g.cov_inflate_circles(g.knot_circle, base, CC.CIRCLE_KAPPA, rpos)  # does not compound
    assert g.get_knot_params(g.knot_circle).tobytes() == par.tobytes()
    # the device variant writes the same track
    db, dr = DeviceBuffer(base.nbytes, base), DeviceBuffer(rpos.nbytes, rpos)
    g.cov_inflate_circles_device(g.knot_circle, db.ptr, base.shape[-2], per_instance, CC.CIRCLE_KAPPA, dr.ptr)
    assert g.get_knot_params(g.knot_circle).tobytes() == par.tobytes()
    db.free()
    dr.free()
    # the solve on the inflated track, from the initial guess again, against the oracle given the same radii per knot
    g.set_trajectory(None, CC.circle_guess(N))
    o = CC.circle_problem(A, P, oracle_make, None, offset, per_knot=par)
    so, _ = _against_the_oracle(A, o, g, f"inflated circle, per_instance {per_instance}, offset {offset}", TIGHT)
    assert (so["status"] == A.SOLVED).all() and (g.get_stats()["status"] == A.SOLVED).all()
    X = g.get_trajectory()[0]
    d2 = (X[:, 1:N, 0] - par[:, :, 0]) ** 2 + (X[:, 1:N, 1] - par[:, :, 1]) ** 2
    tol = g.get_options().constraint_tolerance
    assert (d2 >= par[:, :, 2] ** 2 - tol).all(), (d2 - par[:, :, 2] ** 2).min()
    o.close()
    g.close()


# ---- 10. the asynchronous-solve guard --------------------------------------------------------------------------------------------------
def test_asynchronous_solve_guard(A, P, hip_make):
    """While an asynchronous solve owns the handle all four calls answer ALTRO_NOT_READY, and work again behind altro_wait."""
    base = CC.circle_base()
    s = CC.circle_problem(A, P, hip_make, base)
    s.solve()
    rpos = s.cov_propagate(s.N, CC.CIRCLE_SIGMA0, want=("rpos",))["rpos"]
    s.solve_async()
    for call in (lambda: s.cov_propagate(s.N, CC.CIRCLE_SIGMA0), lambda: s.cov_propagate_device(s.N, 0, False, 0, 0, 8),
                 lambda: s.cov_inflate_circles(s.knot_circle, base, 1.0, rpos),
                 lambda: s.cov_inflate_circles_device(s.knot_circle, 8, base.shape[0], False, 1.0, 8)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.NOT_READY})" in str(e.value)
    s.wait()
    assert s.cov_propagate(s.N, CC.CIRCLE_SIGMA0, want=("rpos",))["rpos"].shape == rpos.shape
    s.close()
