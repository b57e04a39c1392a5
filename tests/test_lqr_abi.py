"""Time-varying LQR tracking gains (include/altro_lqr.h), the parts that need no GPU: the header as C and as C++, the exports,
the binding and the facade, everything that is refused before any device work, and the numpy statement of
tests/_lqr_common.py against plain loops and against what the recursion must satisfy on a linear system."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _lqr_common as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LQR_FUNCTIONS = ("altro_lqr_gains", "altro_lqr_gains_device", "altro_lqr_set_policy", "altro_lqr_get_policy")
LQR_METHODS = ("lqr_gains", "lqr_gains_device", "set_lqr_policy", "get_lqr_policy")
N = 12
EPS = 2.0 ** -52


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


@pytest.mark.parametrize("compiler, std, ext", [("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "cpp")])
def test_header_compiles(tmp_path, compiler, std, ext):
    src = tmp_path / ("lqr." + ext)
    src.write_text('#include "altro_lqr.h"\nint limits(void) { return ALTRO_LQR_MAX_STATES + ALTRO_LQR_MAX_CONTROLS; }\n'
                   "altro_status call(altro_handle h, const double* w, double* o, int* f) { return altro_lqr_gains(h, w, w, 0, 1, o, o, f); }\n")
    r = subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_lqr.h declares the four entry points, the library exports them, include/altro_hip.h (which the oracle
    mirrors function by function) declares none, and the binding and the facade have their calls."""
    lqr, hip = _declared("altro_lqr.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in LQR_FUNCTIONS:
        assert f in lqr and f not in hip and hasattr(lib, f), f
    assert sorted(lqr) == sorted(LQR_FUNCTIONS)
    for method in LQR_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("ComputeLqrGains", "SetLqrGainPolicy", "ClearLqrGainPolicy"):
        assert re.search(r"\b%s\(" % name, facade), name
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "lqr_facade_driver.cpp"))


def _arr(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return (ctypes.c_double * a.size)(*a.ravel())


def test_refusals_without_a_device(A, P):
    B, n, m = 3, 3, 2
    s = P.unicycle_turn90(_make(A), batch=B, N=N)
    lib = A.load_library()
    for f in LQR_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    h = s._h
    Q, R = _arr(np.eye(n)), _arr(np.eye(m))
    K = (ctypes.c_double * (B * N * m * n))()
    Pm = (ctypes.c_double * (B * (N + 1) * n * n))()
    fail = (ctypes.c_int * B)()

    def refused(status, got, word=None, solver=s):
        assert got == status, (got, solver._errmsg(solver._h))
        msg = solver._errmsg(solver._h)
        assert msg, "altro_last_error is empty"
        assert word is None or word in msg, msg

    def gains(Q=Q, R=R, Qf=None, install=0, outs=(K, Pm, fail), handle=h):
        return [lib.altro_lqr_gains(handle, Q, R, Qf, install, *outs), lib.altro_lqr_gains_device(handle, Q, R, Qf, install, *outs)]
    # a NULL handle
    null = ctypes.c_void_p(None)
    assert gains(handle=null) == [A.INVALID_ARG] * 2
    assert lib.altro_lqr_set_policy(null, Q, R, None) == A.INVALID_ARG
    on = ctypes.c_int(7)
    assert lib.altro_lqr_get_policy(null, ctypes.byref(on), None, None, None) == A.INVALID_ARG
    # Q or R NULL
    for st in gains(Q=None) + gains(R=None):
        refused(A.INVALID_ARG, st, "required")
    refused(A.INVALID_ARG, lib.altro_lqr_set_policy(h, Q, None, None), "R")
    # nothing asked for: install == 0 with K and P both NULL (fail alone is nothing)
    for st in gains(outs=(None, None, fail)) + gains(outs=(None, None, None)):
        refused(A.INVALID_ARG, st, "nothing")
    # a non-finite entry in a lower triangle of Q, R or Qf (host arrays: a device caller's are read back first)
    for bad in (float("nan"), float("inf"), -float("inf")):
        for which in ("Q", "R", "Qf"):
            M = np.eye(m if which == "R" else n)
            M[-1, 0] = bad
            kw = {which: _arr(M)}
            refused(A.INVALID_ARG, lib.altro_lqr_gains(h, kw.get("Q", Q), kw.get("R", R), kw.get("Qf"), 0, K, Pm, fail), "finite")
            refused(A.INVALID_ARG, lib.altro_lqr_set_policy(h, kw.get("Q", Q), kw.get("R", R), kw.get("Qf")), "finite")
    # R not positive definite: indefinite, singular, negative (a host Cholesky of its lower triangle)
    for Rbad in (np.array([[1.0, 0.0], [2.0, 1.0]]), np.array([[1.0, 0.0], [1.0, 1.0]]), -np.eye(2), np.zeros((2, 2))):
        refused(A.INVALID_ARG, lib.altro_lqr_gains(h, Q, _arr(Rbad), None, 0, K, Pm, fail), "positive definite")
        refused(A.INVALID_ARG, lib.altro_lqr_gains(h, Q, _arr(Rbad), None, 1, None, None, None), "positive definite")
        refused(A.INVALID_ARG, lib.altro_lqr_set_policy(h, Q, _arr(Rbad), None), "positive definite")
    with pytest.raises(A.AltroError) as e:
        s.lqr_gains(np.eye(n), -np.eye(m))
    assert f"({A.INVALID_ARG})" in str(e.value)
    # ... and only the lower triangle decides: this R is positive definite by its lower triangle, garbage above
    assert lib.altro_lqr_set_policy(h, Q, _arr(np.array([[1.0, 9.0], [0.1, 1.0]])), None) == A.OK
    # the dimensions: more than 8 controls, more than 32 states
    for dims in ((3, 9), (33, 1)):
        big = A.BatchSolver(dims[0], dims[1], N, B, A.F64)
        w = _arr(np.eye(max(dims)))
        for st in gains(Q=w, R=w, handle=big._h):
            refused(A.UNSUPPORTED, st, "supported", solver=big)
        refused(A.UNSUPPORTED, lib.altro_lqr_set_policy(big._h, w, w, None), "supported", solver=big)
        big.close()
    # the policy lives on the handle before any device state exists: set, read back (mirrored lower triangles), clear
    Qp = np.diag([1.0, 2.0, 3.0]) + np.tril(np.full((n, n), 0.1), -1) + np.triu(np.full((n, n), 9.0), 1)
    Rp = np.array([[0.5, 7.0], [0.05, 0.4]])
    assert s.get_lqr_policy() is not None  # (set a few lines up)
    s.set_lqr_policy(None)
    assert s.get_lqr_policy() is None
    s.set_lqr_policy(Qp, Rp)
    got = s.get_lqr_policy()
    sym = lambda M: np.tril(M) + np.tril(M, -1).T  # noqa: E731
    assert (got["Q"] == sym(Qp)).all() and (got["R"] == sym(Rp)).all() and (got["Qf"] == sym(Qp)).all()
    s.set_lqr_policy(Qp, Rp, 10 * Qp)
    assert (s.get_lqr_policy()["Qf"] == sym(10 * Qp)).all()
    s.set_lqr_policy(None)
    assert s.get_lqr_policy() is None
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.lqr_gains(np.eye(2), np.eye(m))
    with pytest.raises(ValueError):
        s.lqr_gains(np.eye(n), np.eye(m), want=("K", "S"))
    with pytest.raises(ValueError):
        s.set_lqr_policy(np.eye(n), np.eye(3))
    s.close()


def test_no_cpu_fallback(A, P):
    """Without a GPU a call that reaches the engine fails with a HIP error -- nothing of the LQR calls succeeds on the host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_lqr_gpu.py covers the other side
    s = P.unicycle_turn90(_make(A), batch=3, N=N)
    for call in (lambda: s.lqr_gains(np.eye(3), np.eye(2)), lambda: s.lqr_gains_device(8, 8, 0, True)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
    s.close()


def test_statement_against_plain_loops():
    """gains of tests/_lqr_common.py against triple loops and numpy's solver on random inputs; only lower triangles are read;
    P is symmetric bit for bit; float64 and longdouble agree to rounding; the root-free factorisation is a factorisation."""
    rng = np.random.RandomState(3)
    B, Nk, n, m = 2, 6, 4, 2
    Am = np.eye(n) + 0.1 * rng.randn(B, Nk, n, n)
    Bm = 0.3 * rng.randn(B, Nk, n, m)
    G = rng.randn(n, n)
    Q, Qf = G @ G.T + np.eye(n), 3.0 * np.eye(n)
    H = rng.randn(m, m)
    R = H @ H.T + 0.5 * np.eye(m)
    K, Pm, fail, kappa = LC.gains(Am, Bm, Q, R, Qf)
    assert K.shape == (B, Nk, m, n) and Pm.shape == (B, Nk + 1, n, n) and (fail == -1).all() and 1.0 <= kappa < 1e3
    assert (Pm == np.swapaxes(Pm, 2, 3)).all()
    for b in range(B):
        Kl, Pl = LC.gains_loops(Am[b], Bm[b], Q, R, Qf)
        assert np.abs(K[b] - Kl).max() <= 1e-12 * np.abs(Kl).max() and np.abs(Pm[b] - Pl).max() <= 1e-12 * np.abs(Pl).max()
    up_n, up_m = np.triu(np.ones((n, n)), 1) * 7.0, np.triu(np.ones((m, m)), 1) * 5.0
    K2, P2, _, _ = LC.gains(Am, Bm, Q + up_n, R - up_m, Qf + up_n)
    assert (K2 == K).all() and (P2 == Pm).all()
    Kq, Pq, _, _ = LC.gains(Am, Bm, Q, R)  # Qf None: Q
    assert (Pq[:, Nk] == Q).all() and (Pm[:, Nk] == Qf).all()
    KL, PL, failL, _ = LC.gains(Am, Bm, Q, R, Qf, dtype=np.longdouble)
    assert KL.dtype == np.longdouble and (failL == -1).all()
    assert np.abs(K - KL).max() < 1e-13 * np.abs(K).max() and np.abs(Pm - PL).max() < 1e-13 * np.abs(Pm).max()
    L, d, ok = LC.ldl(R)
    assert ok and np.abs(L @ np.diag(d) @ L.T - R).max() < 1e-14 * np.abs(R).max() and (np.triu(L, 1) == 0).all()
    x = LC.ldl_solve(L, d, np.eye(m))
    assert np.abs(R @ x - np.eye(m)).max() < 1e-13


def test_triple_integrator_monotone_and_riccati():
    """On the triple integrator's exact A, B (time-invariant, so the recursion is the Riccati difference equation): with
    Qf = 0 the cost-to-go cannot shrink with more knots to go, P_k >= P_{k+1} in the Loewner order; and with N = 400 P_0 has
    reached the fixed point: the residual of the algebraic Riccati equation at P_0 is below n^2 2^-52 |P_0| kappa_S."""
    Ad, Bd = LC.triple_integrator_AB(0.1, 2)
    n, m = 6, 2
    Q = np.diag([1.0, 1.0, 0.5, 0.5, 0.2, 0.2])
    R = np.array([[0.1, 0.0], [0.01, 0.2]])
    Nk = 40
    K, Pm, fail, kappa = LC.gains(np.tile(Ad, (1, Nk, 1, 1)), np.tile(Bd, (1, Nk, 1, 1)), Q, R, np.zeros((n, n)))
    assert fail[0] == -1
    for k in range(Nk):
        D = Pm[0, k] - Pm[0, k + 1]
        assert np.linalg.eigvalsh(D).min() >= -n * n * EPS * np.linalg.norm(Pm[0, k], 2) * max(1.0, kappa), k
    assert np.linalg.eigvalsh(Pm[0, 0] - Pm[0, Nk]).min() > 0.1  # (and it did grow)
    Nk = 400
    K, Pm, fail, kappa = LC.gains(np.tile(Ad, (1, Nk, 1, 1)), np.tile(Bd, (1, Nk, 1, 1)), Q, R, np.zeros((n, n)))
    assert fail[0] == -1
    P0 = Pm[0, 0]
    Rs = np.tril(R) + np.tril(R, -1).T
    S, G = Rs + Bd.T @ P0 @ Bd, Bd.T @ P0 @ Ad
    res = np.linalg.norm(P0 - (Q + Ad.T @ P0 @ Ad - G.T @ np.linalg.solve(S, G)), 2)
    bar = n * n * EPS * np.linalg.norm(P0, 2) * kappa
    print(f"Riccati residual at P_0, N = 400: {res:.3e}, bar {bar:.3e} (kappa_S {kappa:.2f})")
    assert res < bar


def test_indefinite_q_fails_at_a_knot():
    """A Q with a negative eigenvalue large enough drives P negative until S = R + B^T P B loses a pivot: the statement reports
    the knot, everything from there down is NaN and everything above it is finite."""
    Ad, Bd = LC.triple_integrator_AB(0.1, 2)
    n, Nk = 6, 30
    Q = np.diag([1.0, 1.0, 0.5, 0.5, -400.0, 0.2])
    R = 0.1 * np.eye(2)
    A2 = np.tile(Ad, (2, Nk, 1, 1))
    B2 = np.tile(Bd, (2, Nk, 1, 1))
    B2[1] = 0.0  # without control authority S = R: this instance cannot fail
    K, Pm, fail, _ = LC.gains(A2, B2, Q, R, np.eye(n))
    assert 0 <= fail[0] < Nk - 1 and fail[1] == -1
    k = fail[0]
    assert np.isnan(K[0, :k + 1]).all() and np.isnan(Pm[0, :k + 1]).all()
    assert np.isfinite(K[0, k + 1:]).all() and np.isfinite(Pm[0, k + 1:]).all() and np.isfinite(K[1]).all() and np.isfinite(Pm[1]).all()
    assert np.linalg.eigvalsh(Pm[0, k + 1]).min() < 0
    KL, PL, failL, _ = LC.gains(A2, B2, Q, R, np.eye(n), dtype=np.longdouble)
    assert (failL == fail).all()
