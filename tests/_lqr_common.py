"""Shared by tests/test_lqr_abi.py, tests/test_lqr_gpu.py and tests/test_lqr_facade_gpu.py: include/altro_lqr.h stated in numpy.
Every function takes ``dtype`` so that the same code runs in float64 and in np.longdouble (the reference's own rounding
sensitivity is the difference of the two)."""
import json

import numpy as np

from _cov_common import lower_sym, matrix_rel

EPS = 2.0 ** -52


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


def reference(A, Bm, Q, R, Qf):
    """the statement in float64 and in longdouble on the same Jacobians; neither may fail"""
    K, Pm, fail, kappa = gains(A, Bm, Q, R, Qf)
    KL, PL, failL, _ = gains(A, Bm, Q, R, Qf, dtype=np.longdouble)
    assert (fail == -1).all() and (failL == -1).all()
    return dict(K=K, P=Pm, KL=KL, PL=PL, kappa=kappa)


def parity(name, ref, got, N, n, m, fractions, out=None):
    """K and P of one call (``got``: K [B][N][m][n], P [B][N + 1][n][n], fail [B]) against ``ref`` (reference()).  The error of
    a matrix is max |gpu - numpy| / max |numpy| per (instance, knot); its bar is the larger of 8 x the same quantity between
    the float64 and the longdouble run of the statement and 4 N (n + m) 2^-52 max(1, kappa_S).  The largest error as a
    fraction of its bar goes to fractions[name] and, where ``out`` names a file, the whole of ``fractions`` goes there."""
    print(f"{name}: kappa_S {ref['kappa']:.3g}")
    assert ref["kappa"] < 1e3, ref["kappa"]  # (the weights of the parity tests keep the one solve per knot well conditioned)
    floor = 4 * N * (n + m) * EPS * max(1.0, ref["kappa"])
    missed, worst = [], {}
    for key in ("K", "P"):
        r, rl = ref[key], ref[key + "L"]
        assert got[key].shape == r.shape, (key, got[key].shape, r.shape)
        own = (np.abs(r.astype(np.longdouble) - rl).max(axis=(-1, -2))
               / np.maximum(np.abs(rl).max(axis=(-1, -2)), np.longdouble(1e-300))).astype(np.float64)
        bar = np.maximum(8.0 * own, floor)
        err = matrix_rel(got[key], r)
        worst[key] = (float(err.max()), float((err / bar).max()))
        for idx in np.argwhere(~(err <= bar)):
            missed.append((key, tuple(idx), float(err[tuple(idx)]), float(bar[tuple(idx)])))
    print(f"{name}: " + ", ".join(f"{k} err {v[0]:.2e} ({v[1]:.3f} of its bar)" for k, v in worst.items()))
    fractions[name] = {k: v[1] for k, v in worst.items()}
    if out:
        with open(out, "w") as f:
            json.dump(fractions, f, indent=1, sort_keys=True)
    assert not missed, (name, missed[:6])
    assert (got["fail"] == -1).all()


def mixed_failure_qf(A, Bm, Q, R, qf_of):
    """Qf = qf_of(v), indefinite through its one entry -v, with v found by the statement: a coarse sweep brackets the weights
    between "nobody fails" and "everybody fails", a fine one inside the bracket takes the first v at which a quarter to three
    quarters of the instances fail and for which v (1 -+ 1e-6) give the very same fail vector -- no pivot sits within rounding
    of the edge.  -> (Qf, v)"""
    fails_at = lambda v: gains(A, Bm, Q, R, qf_of(v))[2]  # noqa: E731
    coarse = np.geomspace(1.0, 1e4, 41)
    count = [int((fails_at(v) >= 0).sum()) for v in coarse]
    B = A.shape[0]
    lo = max(i for i, v in enumerate(count) if v == 0)
    hi = min(i for i, v in enumerate(count) if v == B)
    assert lo < hi, count
    fine = np.linspace(coarse[lo], coarse[hi], 41)
    for _ in range(4):
        fails = [fails_at(v) for v in fine]
        for v, f in zip(fine, fails):
            if 0.25 * B <= (f >= 0).sum() <= 0.75 * B and (fails_at(v * (1 - 1e-6)) == f).all() and (fails_at(v * (1 + 1e-6)) == f).all():
                return qf_of(v), float(v)
        # a small batch whose instances give way within one fine step of each other (5 instances: from none to 4 of 5 in one
        # step): the same 41 points again between the last v with too few failures and the first with too many
        count = [int((f >= 0).sum()) for f in fails]
        over = min(i for i, v in enumerate(count) if v > 0.75 * B)
        under = max(i for i, v in enumerate(count[:over]) if v < 0.25 * B)
        fine = np.linspace(fine[under], fine[over], 41)
    raise AssertionError(count)


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
