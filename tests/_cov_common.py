"""Shared by tests/test_cov_abi.py, tests/test_cov_gpu.py and tests/test_cov_facade_gpu.py: include/altro_covariance.h stated
in numpy.  Every function takes ``dtype`` so that the same code runs in float64 and in np.longdouble (the reference's own
rounding sensitivity is the difference of the two)."""
import numpy as np

W_PER_INSTANCE, W_PER_KNOT = 1, 2


def lower_sym(M):
    """The symmetric matrices whose lower triangles (i >= j) are those of M [..., n, n]: the upper triangle is never read."""
    L = np.tril(M)
    return L + np.swapaxes(np.tril(M, -1), -1, -2)


def w_of(W, w_mode, b, k, n, dtype):
    """W_k of instance b under w_mode (None: zero)"""
    if W is None:
        return np.zeros((n, n), dtype=dtype)
    W = np.asarray(W)
    if w_mode == 0:
        M = W
    elif w_mode == W_PER_INSTANCE:
        M = W[b]
    elif w_mode == W_PER_KNOT:
        M = W[k]
    else:
        M = W[b, k]
    return lower_sym(M.astype(dtype))


def propagate(A, Bm, K, steps, Sigma0=None, W=None, w_mode=0, dtype=np.float64):
    """A [B][N][n][n], Bm [B][N][n][m], K [B][N][m][n] -> Sigma [B][steps + 1][n][n]:
    Sigma_0 = lower_sym(Sigma0[b]), F_k = A_k + B_k K_k, Sigma_{k+1} = lower_sym(F_k Sigma_k F_k^T + lower_sym(W_k))."""
    A, Bm, K = (np.asarray(a).astype(dtype) for a in (A, Bm, K))
    B, n = A.shape[0], A.shape[2]
    Sigma = np.zeros((B, steps + 1, n, n), dtype=dtype)
    for b in range(B):
        if Sigma0 is not None:
            S0 = np.asarray(Sigma0)
            Sigma[b, 0] = lower_sym((S0[b] if S0.ndim == 3 else S0).astype(dtype))
        for k in range(steps):
            F = A[b, k] + Bm[b, k] @ K[b, k]
            Sigma[b, k + 1] = lower_sym(F @ Sigma[b, k] @ F.T + w_of(W, w_mode, b, k, n, dtype))
    return Sigma


def spreads(Sigma, K, dtype=np.float64):
    """Sigma [B][steps + 1][n][n], K [B][N][m][n] -> sx [B][steps + 1][n], su [B][steps][m], rpos [B][steps + 1]; a negative
    argument of a square root is clamped to zero.  rpos is None for n = 1 (a position is two states)."""
    Sigma, K = np.asarray(Sigma).astype(dtype), np.asarray(K).astype(dtype)
    steps = Sigma.shape[1] - 1
    root = lambda v: np.sqrt(np.maximum(v, dtype(0)))  # noqa: E731
    sx = root(np.diagonal(Sigma, axis1=2, axis2=3))
    Kk = K[:, :steps]
    su = root(np.einsum("bkia,bkac,bkic->bki", Kk, Sigma[:, :steps], Kk))
    if Sigma.shape[2] < 2:
        return sx, su, None
    a, b, c = Sigma[:, :, 0, 0], Sigma[:, :, 1, 0], Sigma[:, :, 1, 1]
    rpos = root((a + c) / 2 + np.sqrt(((a - c) / 2) ** 2 + b ** 2))
    return sx, su, rpos


def inflate(base, batch, kappa, rpos, offset, N, dtype=np.float64):
    """base [rows][3 nobs] or [B][rows][3 nobs], rpos [B][N + 1] -> the track [B][rows][3 nobs]: cx, cy kept,
    radius + kappa * rpos[b][min(max(r - offset, 0), N)]."""
    base = np.asarray(base).astype(dtype)
    out = np.array(np.broadcast_to(base, (batch,) + base.shape[-2:]))
    rows = out.shape[1]
    at = np.clip(np.arange(rows) - offset, 0, N)
    out[:, :, 2::3] = out[:, :, 2::3] + dtype(kappa) * np.asarray(rpos).astype(dtype)[:, at][:, :, None]
    return out


def matrix_rel(got, want):
    """max |got - want| / max |want| per matrix (the last two axes); 0 where both are zero"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = np.abs(got - want).max(axis=(-1, -2))
    scale = np.abs(want).max(axis=(-1, -2))
    return np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), err)


# ---- the inflation scenario (tests/test_cov_gpu.py test 9; tests/test_cov_abi.py solves it on the oracle) --------------------------------------
# problems.unicycle_turn90 (control bound, goal constraint) with N = 12, batch 3, a different x0 per instance, and ONE knot
# circle constraint with one circle on [1, N).  The base track has 8 rows, fewer than the window of 13: the last row is held.
# The circle lies beside the turn and drifts towards it from row to row; inflated by kappa * rpos it pushes the plan outwards.
CIRCLE_N, CIRCLE_B, CIRCLE_ROWS = 12, 3, 8
CIRCLE_SIGMA0 = np.diag([4e-4, 4e-4, 1e-4])
CIRCLE_W = np.diag([1e-5, 1e-5, 1e-6])
CIRCLE_KAPPA = 2.0


def circle_x0():
    b = np.arange(CIRCLE_B, dtype=np.float64)
    return np.stack([0.05 * b, -0.04 * b, 0.03 * b], axis=1)


def circle_base(batch=0):
    """[rows][3], or [batch][rows][3]: centre (1.25 - 0.01 r, 0.30 + 0.01 r) (+ 0.02 b on x), radius 0.20 (+ 0.01 b)"""
    r = np.arange(CIRCLE_ROWS, dtype=np.float64)
    one = np.stack([1.25 - 0.01 * r, 0.30 + 0.01 * r, np.full(CIRCLE_ROWS, 0.20)], axis=1)
    if not batch:
        return one
    out = np.repeat(one[None], batch, axis=0)
    out[:, :, 0] += 0.02 * np.arange(batch)[:, None]
    out[:, :, 2] += 0.01 * np.arange(batch)[:, None]
    return out


def circle_guess(N=CIRCLE_N):
    return np.tile(np.array([0.1, 0.1]), (N, 1))


def circle_problem(A, P, make, base, offset=0, per_knot=None):
    """The device's form: the knot constraint with the track ``base`` and the window at ``offset``.  ``per_knot`` [B][N - 1][3]:
    the reference's idiom instead (what the CPU oracle takes) -- one ordinary circle constraint per knot of [1, N) with these
    parameters per instance."""
    N, B = CIRCLE_N, CIRCLE_B
    s = P.unicycle_turn90(make, batch=B, N=N)
    s.set_initial_state(circle_x0())
    if per_knot is not None:
        for k in range(1, N):
            s.add_constraint(A.CON_CIRCLE, k, k + 1, np.ascontiguousarray(per_knot[:, k - 1]))
    else:
        s.knot_circle = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 3)
        s.set_constraint_track(s.knot_circle, base)
        if offset:
            s.set_track_offset(offset)
    return s
