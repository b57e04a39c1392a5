"""Closed-loop covariance (include/altro_covariance.h), the parts that need no GPU: the header as C, the exports, everything
that is refused before any device work, and the numpy statements of tests/_cov_common.py against plain loops."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _cov_common as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_FUNCTIONS = ("altro_cov_propagate", "altro_cov_propagate_device", "altro_cov_inflate_circles", "altro_cov_inflate_circles_device")
COV_METHODS = ("cov_propagate", "cov_propagate_device", "cov_inflate_circles", "cov_inflate_circles_device")
N = 12


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "cov.c"
    src.write_text('#include "altro_covariance.h"\nint modes(void) { return ALTRO_COV_W_PER_INSTANCE | ALTRO_COV_W_PER_KNOT; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_covariance.h declares the four entry points, the library exports them, include/altro_hip.h (which the
    oracle mirrors function by function) declares none, and the binding and the facade have their calls."""
    cov, hip = _declared("altro_covariance.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in COV_FUNCTIONS:
        assert f in cov and f not in hip and hasattr(lib, f), f
    assert sorted(cov) == sorted(COV_FUNCTIONS)
    for method in COV_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    assert (A.COV_W_PER_INSTANCE, A.COV_W_PER_KNOT) == (1, 2) == (CC.W_PER_INSTANCE, CC.W_PER_KNOT)
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("PropagateCovariance", "InflateCircleTrack"):
        assert re.search(r"\b%s\(" % name, facade), name


def test_refusals_without_a_device(A, P):
    B = 3
    s = P.moving_obstacles(_make(A), batch=B, N=N)
    lib = A.load_library()
    for f in COV_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    dbl = ctypes.c_double
    n = 3
    S0 = (dbl * (n * n))(*np.eye(n).ravel())
    out = (dbl * (B * (N + 1) * n * n))()
    base = (dbl * (2 * 6))(*([0.5, 0.5, 0.1] * 4))
    rpos = (dbl * (B * (N + 1)))()
    h = s._h

    def refused(status, got, word=None):
        assert got == status, (got, s._errmsg(h))
        msg = s._errmsg(h)
        assert msg, "altro_last_error is empty"
        assert word is None or word in msg, msg

    def propagate(steps=N, w_mode=0, outs=(out, None, None, None), handle=h):
        return [lib.altro_cov_propagate(handle, steps, S0, 0, None, w_mode, *outs),
                lib.altro_cov_propagate_device(handle, steps, S0, 0, None, w_mode, *outs)]

    def inflate(index, base=base, rows=2, kappa=2.0, rpos=rpos, handle=h):
        return [lib.altro_cov_inflate_circles(handle, index, base, rows, 0, dbl(kappa), rpos),
                lib.altro_cov_inflate_circles_device(handle, index, base, rows, 0, dbl(kappa), rpos)]
    # steps outside [1, N]
    for bad in (0, -1, N + 1):
        for st in propagate(steps=bad):
            refused(A.INVALID_ARG, st, "steps")
    # all four outputs NULL
    for st in propagate(outs=(None, None, None, None)):
        refused(A.INVALID_ARG, st)
    # w_mode outside 0..3
    for bad in (-1, 4, 7):
        for st in propagate(w_mode=bad):
            refused(A.INVALID_ARG, st, "w_mode")
    # no backward pass has left gains on the handle (every argument valid)
    for mode in range(4):
        for st in propagate(w_mode=mode):
            refused(A.NOT_READY, st, "gains")
    # rpos asked for with n < 2
    one = A.BatchSolver(1, 1, N, B, A.F64)
    for st in propagate(outs=(None, None, None, rpos), handle=one._h):
        assert st == A.INVALID_ARG and "rpos" in one._errmsg(one._h)
    one.close()
    # index: out of range, an ordinary constraint, a knot constraint that is no circle
    plain = P.unicycle_turn90(_make(A), batch=B, N=N)
    for st in inflate(0, handle=plain._h):
        assert st == A.INVALID_ARG and "knot constraint" in plain._errmsg(plain._h)
    plain.close()
    for bad in (-1, 99, s.knot_bound):
        for st in inflate(bad):
            refused(A.INVALID_ARG, st)
    # rows < 1, kappa negative or not finite, rpos or base NULL
    for bad in (0, -2):
        for st in inflate(s.knot_circle, rows=bad):
            refused(A.INVALID_ARG, st, "row")
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        for st in inflate(s.knot_circle, kappa=bad):
            refused(A.INVALID_ARG, st, "kappa")
    for st in inflate(s.knot_circle, base=None) + inflate(s.knot_circle, rpos=None):
        refused(A.INVALID_ARG, st)
    # a NULL handle
    null = ctypes.c_void_p(None)
    assert propagate(handle=null) == [A.INVALID_ARG] * 2 and inflate(s.knot_circle, handle=null) == [A.INVALID_ARG] * 2
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.cov_propagate(N, Sigma0=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        s.cov_propagate(N, W=np.zeros((N + 1, 3, 3)))
    with pytest.raises(ValueError):
        s.cov_propagate(N, want=("Sigma", "sy"))
    with pytest.raises(ValueError):
        s.cov_inflate_circles(s.knot_circle, np.zeros((2, 6)), 1.0, np.zeros((B, N)))
    with pytest.raises(ValueError):
        s.cov_inflate_circles(s.knot_circle, np.zeros((2, 5)), 1.0, np.zeros((B, N + 1)))
    s.close()


def test_no_cpu_fallback(A, P):
    """Without a GPU a call that reaches the engine fails with a HIP error -- nothing of the covariance calls succeeds on the
    host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_cov_gpu.py covers the other side
    s = P.moving_obstacles(_make(A), batch=3, N=N)
    base = np.tile([0.5, 0.5, 0.1], (2, 2))
    for call in (lambda: s.cov_inflate_circles(s.knot_circle, base, 2.0, np.zeros((3, N + 1))),
                 lambda: s.cov_inflate_circles_device(s.knot_circle, 8, 2, False, 2.0, 8)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
    s.close()


def _random_case(rng, B, Nk, n, m):
    Am = np.eye(n) + 0.1 * rng.randn(B, Nk, n, n)
    Bm = 0.1 * rng.randn(B, Nk, n, m)
    K = rng.randn(B, Nk, m, n)
    return Am, Bm, K


def test_numpy_statements():
    """propagate, spreads and inflate of tests/_cov_common.py against plain loops on random inputs; only lower triangles are
    read; Sigma stays symmetric bit for bit and, for PSD inputs, PSD to rounding; float64 and longdouble agree to rounding."""
    rng = np.random.RandomState(5)
    B, Nk, n, m, steps = 2, 5, 4, 2, 4
    Am, Bm, K = _random_case(rng, B, Nk, n, m)
    G = rng.randn(B, n, n)
    S0 = G @ np.swapaxes(G, 1, 2)
    H = 0.1 * rng.randn(B, steps, n, n)
    W = H @ np.swapaxes(H, 2, 3)
    for w_mode, Wm in ((0, W[0, 0]), (CC.W_PER_INSTANCE, W[:, 0]), (CC.W_PER_KNOT, W[0]), (3, W), (0, None)):
        for S0m in (S0, S0[0], None):
            Sig = CC.propagate(Am, Bm, K, steps, S0m, Wm, w_mode)
            assert Sig.shape == (B, steps + 1, n, n) and (Sig == np.swapaxes(Sig, 2, 3)).all()
            for b in range(B):
                S = np.zeros((n, n)) if S0m is None else (S0m[b] if S0m.ndim == 3 else S0m).copy()
                for k in range(steps + 1):
                    assert np.abs(Sig[b, k] - S).max() <= 1e-13 * max(np.abs(S).max(), 1.0), (w_mode, b, k)
                    assert np.linalg.eigvalsh(Sig[b, k]).min() >= -1e-13 * max(np.abs(S).max(), 1.0)
                    if k == steps:
                        break
                    F = np.zeros((n, n))
                    for i in range(n):
                        for j in range(n):
                            F[i, j] = Am[b, k, i, j] + sum(Bm[b, k, i, c] * K[b, k, c, j] for c in range(m))
                    Wk = np.zeros((n, n)) if Wm is None else {0: lambda: Wm, 1: lambda: Wm[b], 2: lambda: Wm[k], 3: lambda: Wm[b, k]}[w_mode]()
                    S = F @ S @ F.T + Wk
            # garbage above the diagonal of the inputs changes nothing
            if S0m is not None and Wm is not None:
                up = np.triu(np.ones((n, n)), 1) * 7.0
                assert (CC.propagate(Am, Bm, K, steps, S0m + up, Wm - up, w_mode) == Sig).all()
    Sig = CC.propagate(Am, Bm, K, steps, S0, W, 3)
    sx, su, rpos = CC.spreads(Sig, K)
    assert sx.shape == (B, steps + 1, n) and su.shape == (B, steps, m) and rpos.shape == (B, steps + 1)
    for b in range(B):
        for k in range(steps + 1):
            assert np.allclose(sx[b, k], np.sqrt(np.diag(Sig[b, k])), rtol=1e-15, atol=0)
            assert abs(rpos[b, k] - np.sqrt(np.linalg.eigvalsh(Sig[b, k, :2, :2]).max())) <= 1e-14 * rpos[b, k]
            if k < steps:
                assert np.allclose(su[b, k], np.sqrt(np.diag(K[b, k] @ Sig[b, k] @ K[b, k].T)), rtol=1e-14, atol=0)
    # the clamp
    neg = -np.eye(n)[None, None]
    sxn, sun, rn = CC.spreads(neg, K[:1, :0])
    assert (sxn == 0).all() and (rn == 0).all() and sun.shape == (1, 0, m)
    # longdouble against float64: rounding only
    SigL = CC.propagate(Am, Bm, K, steps, S0, W, 3, dtype=np.longdouble)
    assert SigL.dtype == np.longdouble and CC.matrix_rel(Sig, SigL).max() < 1e-14
    # inflate
    rows, offset = 4, 2
    base = rng.rand(rows, 6)
    rp = rng.rand(B, Nk + 1)
    for bs in (base, np.stack([base, base + 1.0])):
        out = CC.inflate(bs, B, 1.5, rp, offset, Nk)
        for b in range(B):
            src = bs[b] if bs.ndim == 3 else bs
            for r in range(rows):
                at = min(max(r - offset, 0), Nk)
                for i in range(2):
                    assert out[b, r, 3 * i] == src[r, 3 * i] and out[b, r, 3 * i + 1] == src[r, 3 * i + 1]
                    assert out[b, r, 3 * i + 2] == src[r, 3 * i + 2] + 1.5 * rp[b, at]


def test_inflation_scenario_solves_on_the_oracle(A, P, oracle_make):
    """The scenario of tests/test_cov_gpu.py's inflation test, on the CPU oracle alone: with the radii inflated by the oracle's
    own covariance (its expansions and gains through the numpy statement) every instance ends ALTRO_SOLVED, for a shared and a
    per-instance base and for both window offsets; and the inflated circle is active on some instance (it matters)."""
    N, B = CC.CIRCLE_N, CC.CIRCLE_B
    knots = np.arange(1, N)
    for per_instance in (False, True):
        for offset in (0, 2):
            base = CC.circle_base(B if per_instance else 0)
            full = np.broadcast_to(base, (B,) + base.shape[-2:])
            o = CC.circle_problem(A, P, oracle_make, None, offset, per_knot=full[:, np.minimum(offset + knots, full.shape[1] - 1)])
            o.solve()
            assert (o.get_stats()["status"] == A.SOLVED).all()
            K = o.get_gains()[0]
            o.update_expansions()
            ex = [o.get_expansion(k) for k in range(N)]
            o.close()
            Sigma = CC.propagate(np.stack([e["A"] for e in ex], axis=1), np.stack([e["B"] for e in ex], axis=1), K, N, CC.CIRCLE_SIGMA0,
                                 CC.CIRCLE_W, 0)
            rpos = CC.spreads(Sigma, K)[2]
            assert rpos.min() > 1e-3 and rpos.max() < 0.1
            track = CC.inflate(base, B, CC.CIRCLE_KAPPA, rpos, offset, N)
            par = track[:, np.minimum(offset + knots, track.shape[1] - 1)]
            o = CC.circle_problem(A, P, oracle_make, None, offset, per_knot=par)
            o.solve()
            st = o.get_stats()
            X = o.get_trajectory()[0]
            o.close()
            assert (st["status"] == A.SOLVED).all(), (per_instance, offset, st["status"])
            gap = np.sqrt((X[:, 1:N, 0] - par[:, :, 0]) ** 2 + (X[:, 1:N, 1] - par[:, :, 1]) ** 2) - par[:, :, 2]
            assert gap.min() < 0.01, (per_instance, offset, gap.min())
