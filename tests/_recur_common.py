"""Shared by tests/test_recur_shapes_gpu.py and tests/test_recur_kernels_gpu.py: the per-instance plans of the shape chain, its
Jacobians by central differences in numpy, the indefinite terminal weight of the failure tests, the layouts of k_lqr_recur
and k_cov_recur, and the record of the measured errors as fractions of their bars (profiles/recur_shapes_parity.json)."""
import json
import os

import numpy as np

import _lqr_common as LC
from _cov_common import lower_sym

N = 24
H = float(np.float32(0.05))  # the step a handle holds after set_uniform_step(np.float32(0.05))


def plan(n, m, B):
    """x0 [B][n] uniform in [-1, 1]^n and one constant control per instance [B][m] uniform in [-0.5, 0.5]^m, drawn instance by
    instance from default_rng(10 n + m): instance b has the same plan whatever the batch."""
    rng = np.random.default_rng(10 * n + m)
    x0, u = np.zeros((B, n)), np.zeros((B, m))
    for b in range(B):
        x0[b] = rng.uniform(-1.0, 1.0, n)
        u[b] = rng.uniform(-0.5, 0.5, m)
    return x0, u


def chain_jacobians(n, m, B, step=None, eps=1e-6):
    """The plan of ``plan`` rolled out with ``step`` (tests/test_model_shapes_gpu.py: chain_rk4) and its Jacobians by central
    differences of that step -> X [B][N + 1][n], U [B][N][m], A [B][N][n][n], Bm [B][N][n][m].  Inputs of the kernel tests:
    the statement and the kernel are given the same arrays, so the differences' own error does not enter a comparison."""
    if step is None:
        from test_model_shapes_gpu import chain_rk4
        step = lambda x, u: chain_rk4(x, u[:, None, :], H, n, m)  # noqa: E731
    x0, u = plan(n, m, B)
    X, U = np.zeros((B, N + 1, n)), np.repeat(u[:, None, :], N, axis=1)
    A, Bm = np.zeros((B, N, n, n)), np.zeros((B, N, n, m))
    X[:, 0] = x0
    for k in range(N):
        X[:, k + 1] = step(X[:, k], u)
        for j in range(n + m):
            d = np.zeros((1, n + m))
            d[0, j] = eps
            col = (step(X[:, k] + d[:, :n], u + d[:, n:]) - step(X[:, k] - d[:, :n], u - d[:, n:])) / (2 * eps)
            if j < n:
                A[:, k, :, j] = col
            else:
                Bm[:, k, :, j - n] = col
    return X, U, A, Bm


def failure_qf(n):
    """v -> Qf = diag(1, .., 1, 50, -v) cut to its last n entries: -v on state n - 1, the state control 0 of the chain drives"""
    return lambda v: np.diag(np.concatenate([np.ones(n), [50.0, -v]])[-n:])


def check_failure(got, K, Pm, fail):
    """one call with a mixed-failure Qf against the statement's K, P (NaN from the failing knot down) and fail"""
    assert (got["fail"] == fail).all(), (got["fail"], fail)
    assert (np.isnan(got["K"]) == np.isnan(K)).all() and (np.isnan(got["P"]) == np.isnan(Pm)).all()
    for b in np.flatnonzero(fail >= 0):
        assert np.isnan(got["K"][b, :fail[b] + 1]).all() and np.isfinite(got["K"][b, fail[b] + 1:]).all()
        assert np.isnan(got["P"][b, :fail[b] + 1]).all() and np.isfinite(got["P"][b, fail[b] + 1:]).all()
    fine = ~np.isnan(Pm)
    scale = np.abs(Pm[fine]).max()
    assert np.abs(got["P"][fine] - Pm[fine]).max() <= 1e-9 * scale


def mixed_failure(A, Bm, Q, R, n, tag):
    """-> (Qf, K, P, fail) of the statement, fail the same in float64 and longdouble"""
    Qf, v = LC.mixed_failure_qf(A, Bm, Q, R, failure_qf(n))
    K, Pm, fail, _ = LC.gains(A, Bm, Q, R, Qf)
    assert (LC.gains(A, Bm, Q, R, Qf, dtype=np.longdouble)[2] == fail).all()
    print(f"{tag}: v = {v:.5g}: {int((fail >= 0).sum())} of {len(fail)} instances fail, at knots {sorted(set(fail[fail >= 0].tolist()))}")
    return Qf, K, Pm, fail


# ---- the layouts of k_lqr_recur and k_cov_recur (altro_kernels.hpp): the instance is the fastest index, Bp instances a row ------
def padded(B):
    """B rounded up to 64, plus 64"""
    return (B + 63) // 64 * 64 + 64


def instance_fastest(a, Bp, fill):
    """[B][...] -> [...][Bp] with ``fill`` in the columns b >= B"""
    a = np.asarray(a, dtype=np.float64)
    out = np.full(a.shape[1:] + (Bp,), fill, dtype=np.float64)
    out[..., :a.shape[0]] = np.moveaxis(a, 0, -1)
    return np.ascontiguousarray(out)


def pack_AB(A, Bm, Bp):
    """AB[(k n (n + m) + e) Bp + b], e = l + j n of the column-major n x (n + m) matrix [A | B]: [N][n + m][n][Bp]"""
    return instance_fastest(np.swapaxes(np.concatenate([A, Bm], axis=3), 2, 3), Bp, np.nan)


def pack_weights(Q, R, Qf):
    """Q | R | Qf, each full symmetric"""
    return np.concatenate([lower_sym(np.asarray(M, dtype=np.float64)).ravel() for M in (Q, R, Qf)])


def unpack_K(Kt, B):
    """Kt[(k m n + i m + a) Bp + b] = K[a][i], [N][n][m][Bp] -> K [B][N][m][n]"""
    return np.ascontiguousarray(np.moveaxis(Kt[..., :B], -1, 0).swapaxes(2, 3))


def unpack_P(Pt, B):
    """Pt[(k n n + i n + l) Bp + b], [N + 1][n][n][Bp] -> P [B][N + 1][n][n]"""
    return np.ascontiguousarray(np.moveaxis(Pt[..., :B], -1, 0))


# ---- the record ---------------------------------------------------------------------------------------------------------------
FRACTIONS = {}


def record(key, fractions):
    """FRACTIONS[key] = the largest errors of one comparison as fractions of their bars; with ALTRO_RECUR_PARITY_OUT set the
    whole record goes to that file (how profiles/recur_shapes_parity.json is made)"""
    FRACTIONS[key] = {k: max(float(v), FRACTIONS.get(key, {}).get(k, 0.0)) for k, v in fractions.items()}
    if os.environ.get("ALTRO_RECUR_PARITY_OUT"):
        with open(os.environ["ALTRO_RECUR_PARITY_OUT"], "w") as f:
            json.dump(FRACTIONS, f, indent=1, sort_keys=True)
