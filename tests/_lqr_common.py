"""Shared by tests/test_lqr_abi.py, tests/test_lqr_gpu.py and tests/test_lqr_facade_gpu.py: include/altro_lqr.h stated in numpy.
Every function takes ``dtype`` so that the same code runs in float64 and in np.longdouble (the reference's own rounding
sensitivity is the difference of the two)."""
import numpy as np

from _cov_common import lower_sym


def ldl(S, dtype=np.float64):
    """The Cholesky factorisation of the lower triangles of S [...][m][m] without its square roots, S = L D L^T -> (L unit
    lower, d [...][m], ok [...]); ok is False where a pivot is not positive (the factorisation goes on regardless, as the
    kernel's does)."""
    S = np.asarray(S).astype(dtype)
    m = S.shape[-1]
    L = np.zeros(S.shape, dtype=dtype)
    L[..., np.arange(m), np.arange(m)] = 1
    d = np.zeros(S.shape[:-1], dtype=dtype)
    ok = np.ones(S.shape[:-2], dtype=bool)
    with np.errstate(all="ignore"):
        for c in range(m):
            ld = L[..., c, :c] * d[..., :c]
            d[..., c] = S[..., c, c] - (L[..., c, :c] * ld).sum(axis=-1)
            ok &= d[..., c] > 0
            for a in range(c + 1, m):
                L[..., a, c] = (S[..., a, c] - (L[..., a, :c] * ld).sum(axis=-1)) / d[..., c]
    return L, d, ok


def ldl_solve(L, d, rhs, dtype=np.float64):
    """x with (L D L^T) x = rhs [...][m][cols]"""
    m = L.shape[-1]
    x = np.array(rhs, dtype=dtype)
    with np.errstate(all="ignore"):
        for a in range(m):
            x[..., a, :] = x[..., a, :] - (L[..., a, :a, None] * x[..., :a, :]).sum(axis=-2)
        x = x / d[..., :, None]
        for a in range(m - 1, -1, -1):
            x[..., a, :] = x[..., a, :] - (L[..., a + 1:, a, None] * x[..., a + 1:, :]).sum(axis=-2)
    return x


def gains(A, Bm, Q, R, Qf=None, dtype=np.float64):
    """A [B][N][n][n], Bm [B][N][n][m], Q [n][n], R [m][m], Qf [n][n] (None: Q), lower triangles ->
    K [B][N][m][n], P [B][N + 1][n][n], fail [B], kappa_S:
        P_N = Qf;  S = R + B^T P B, G = B^T P A, K_k = -S^-1 G (S = L D L^T), P_k = lower_sym(Q + A^T P A + G^T K_k).
    fail[b] is -1, or the largest k at which a pivot of S_k was not positive or a value of K_k or P_k was not finite; K and P of
    that instance from that knot down are NaN.  kappa_S is the largest 2-norm condition number of an S_k of an instance that
    had not failed by then (in float64).  The batch is one numpy axis: every instance sees the same operations."""
    A, Bm = np.asarray(A).astype(dtype), np.asarray(Bm).astype(dtype)
    Qs, Rs = lower_sym(np.asarray(Q).astype(dtype)), lower_sym(np.asarray(R).astype(dtype))
    Qfs = Qs if Qf is None else lower_sym(np.asarray(Qf).astype(dtype))
    B, N, n, m = A.shape[0], A.shape[1], A.shape[2], Bm.shape[3]
    K = np.zeros((B, N, m, n), dtype=dtype)
    P = np.zeros((B, N + 1, n, n), dtype=dtype)
    fail = np.full(B, -1, dtype=np.int32)
    kappa = 0.0
    T = lambda M: np.swapaxes(M, -1, -2)  # noqa: E731
    with np.errstate(all="ignore"):
        P[:, N] = Qfs
        for k in range(N - 1, -1, -1):
            Ak, Bk = A[:, k], Bm[:, k]
            W = P[:, k + 1] @ np.concatenate([Ak, Bk], axis=2)
            S = Rs + T(Bk) @ W[:, :, n:]
            G = T(Bk) @ W[:, :, :n]
            L, d, ok = ldl(S, dtype)
            Kk = ldl_solve(L, d, -G, dtype)
            Pk = lower_sym(Qs + T(Ak) @ W[:, :, :n] + T(G) @ Kk)
            ok = ok & np.isfinite(Kk.astype(np.float64)).all(axis=(1, 2)) & np.isfinite(Pk.astype(np.float64)).all(axis=(1, 2))
            fail[~ok & (fail < 0)] = k
            dead = fail >= 0
            Kk[dead], Pk[dead] = np.nan, np.nan
            K[:, k], P[:, k] = Kk, Pk
            if (~dead).any():
                kappa = max(kappa, float(np.linalg.cond(lower_sym(S[~dead]).astype(np.float64)).max()))
    return K, P, fail, kappa


def gains_loops(A, Bm, Q, R, Qf=None):
    """The same recursion for ONE instance (A [N][n][n], Bm [N][n][m]) in plain triple loops and numpy's own solver, float64:
    what tests/test_lqr_abi.py holds the statement against.  -> K [N][m][n], P [N + 1][n][n]"""
    N, n, m = A.shape[0], A.shape[1], Bm.shape[2]
    sym = lambda M: np.array([[M[max(i, j)][min(i, j)] for j in range(len(M))] for i in range(len(M))], dtype=np.float64)  # noqa: E731
    Qs, Rs = sym(Q), sym(R)
    P = np.zeros((N + 1, n, n))
    K = np.zeros((N, m, n))
    P[N] = Qs if Qf is None else sym(Qf)
    for k in range(N - 1, -1, -1):
        PA, PB = np.zeros((n, n)), np.zeros((n, m))
        for i in range(n):
            for j in range(n):
                PA[i, j] = sum(P[k + 1, i, l] * A[k, l, j] for l in range(n))
            for j in range(m):
                PB[i, j] = sum(P[k + 1, i, l] * Bm[k, l, j] for l in range(n))
        S, G, APA = np.zeros((m, m)), np.zeros((m, n)), np.zeros((n, n))
        for a in range(m):
            for c in range(m):
                S[a, c] = Rs[a, c] + sum(Bm[k, l, a] * PB[l, c] for l in range(n))
            for c in range(n):
                G[a, c] = sum(Bm[k, l, a] * PA[l, c] for l in range(n))
        for i in range(n):
            for j in range(n):
                APA[i, j] = sum(A[k, l, i] * PA[l, j] for l in range(n))
        K[k] = -np.linalg.solve(S, G)
        for i in range(n):
            for j in range(n):
                P[k, i, j] = Qs[i, j] + APA[i, j] + sum(G[a, i] * K[k, a, j] for a in range(m))
    return K, P


def rollout_cost(A, Bm, K, Q, R, Qf, dx0, dtype=np.float64):
    """One instance: e_0 = dx0, du_k = K_k e_k, e_{k+1} = A_k e_k + B_k du_k ->
    (terms [2 N + 1] of e^T Q e, du^T R du per knot and e_N^T Qf e_N, E [N + 1][n], dU [N][m])"""
    A, Bm, K = (np.asarray(a).astype(dtype) for a in (A, Bm, K))
    Qs, Rs, Qfs = (lower_sym(np.asarray(M).astype(dtype)) for M in (Q, R, Qf))
    N = A.shape[0]
    e = np.asarray(dx0).astype(dtype)
    E, dU, terms = [e], [], []
    for k in range(N):
        du = K[k] @ e
        terms += [e @ Qs @ e, du @ Rs @ du]
        e = A[k] @ e + Bm[k] @ du
        E.append(e)
        dU.append(du)
    terms.append(e @ Qfs @ e)
    return np.array(terms, dtype=dtype), np.array(E, dtype=dtype), np.array(dU, dtype=dtype)


def logged_cost(E, dU, Q, R, Qf, dtype=np.float64):
    """the terms of rollout_cost from logged deviations E [N + 1][n], dU [N][m]"""
    E, dU = np.asarray(E).astype(dtype), np.asarray(dU).astype(dtype)
    Qs, Rs, Qfs = (lower_sym(np.asarray(M).astype(dtype)) for M in (Q, R, Qf))
    terms = []
    for k in range(dU.shape[0]):
        terms += [E[k] @ Qs @ E[k], dU[k] @ Rs @ dU[k]]
    terms.append(E[-1] @ Qfs @ E[-1])
    return np.array(terms, dtype=dtype)


def parity_weights(n, m):
    """The weights of the parity tests: Q = diag in [0.5, 2], R = diag in [0.1, 1] plus a small symmetric off-diagonal part,
    Qf = 10 Q; garbage above the diagonals, which is never read."""
    Q = np.diag(np.linspace(0.5, 2.0, n)) if n > 1 else np.array([[1.0]])
    R = np.diag(np.linspace(0.1, 1.0, m)) if m > 1 else np.array([[0.3]])
    off = 0.01 * np.fromfunction(lambda i, j: 1.0 + np.minimum(i, j), (m, m))
    R = R + np.tril(off, -1) + np.tril(off, -1).T
    Qf = 10.0 * Q
    return Q + np.triu(np.ones((n, n)), 1) * 5.0, R - np.triu(np.ones((m, m)), 1) * 3.0, Qf + np.triu(np.ones((n, n)), 1) * 7.0


def triple_integrator_AB(h=0.1, dof=2):
    """The exact discretisation of the triple integrator (position, velocity, acceleration per degree of freedom; the jerk is
    the control) over a step h: states ordered [positions, velocities, accelerations]."""
    I, Z = np.eye(dof), np.zeros((dof, dof))
    A = np.block([[I, h * I, h * h / 2 * I], [Z, I, h * I], [Z, Z, I]])
    Bm = np.concatenate([h ** 3 / 6 * I, h * h / 2 * I, h * I], axis=0)
    return A, Bm
