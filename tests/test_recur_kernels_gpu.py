"""k_lqr_recur and k_cov_recur driven on their own (tests/cpp/recur_driver.hip) at the lane groups no model of the suite
reaches, against the numpy statements (tests/_lqr_common.py, tests/_cov_common.py) under the bars of tests/test_lqr_gpu.py and
tests/test_cov_gpu.py:

  (2, 6)   G = 2, m > n              (4, 8)   m = 8 > n: the 36-entry packed S on narrow groups
  (8, 1)   n = G = 8, no dead lane   (16, 4)  n = G = 16
  (17, 2)  G = 32 with 15 dead lanes (24, 3)  G = 32, m = 3
  (32, 8)  n = G = 32: both documented maxima; k_lqr_recur spills to scratch there (profiles/recur_shapes_resources.txt)
  (13, 2)  a shape a plug-in reaches too: the driver on the [A | B] of tests/test_recur_shapes_gpu.py's case

A plug-in of 17 states or more takes many minutes to compile, so these shapes have no model; the recursions are templates over
(n, m) alone.  The inputs are the Jacobians of the shape chain by central differences in numpy at the per-instance plans of
tests/_recur_common.py (the statement and the kernel get the same arrays), N = 24, B = 67 where G <= 16 (several workgroups,
the last one partly filled) and B = 5 where G = 32 (3 workgroups, the last half full).  The batch is padded to Bp = B rounded
up to 64, plus 64: the input columns b >= B hold NaN, the outputs are filled with -77 beforehand; nothing at b >= B may be
written and no NaN may reach an instance b < B."""
import ctypes
import os
import sys

import numpy as np
import pytest

import _lqr_common as LC
import _recur_common as RC
from test_cov_gpu import _check as cov_check
from test_cov_gpu import _inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

pytestmark = pytest.mark.gpu

N = RC.N
SHAPES = [(2, 6), (4, 8), (8, 1), (16, 4), (17, 2), (24, 3), (32, 8)]  # smallest group first
CANARY = -77.0


def _ids(shapes):
    return [f"{n}_{m}" for n, m in shapes]


def _batch(n):
    return 67 if n <= 16 else 5


@pytest.fixture(scope="module")
def driver():
    path = os.path.join(ROOT, "tests", "cpp", "librecur_driver.so")
    if not os.path.exists(path):
        graft.build_recur_driver()
    lib = ctypes.CDLL(path)
    lib.recur_lqr.restype = ctypes.c_int
    lib.recur_lqr.argtypes = [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3
    lib.recur_cov.restype = ctypes.c_int
    lib.recur_cov.argtypes = ([ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
                              + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4)
    return lib


def _ptr(a):
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(ctypes.c_void_p)


_INPUTS = {}


def inputs(n, m):
    """-> dict(A, B: the Jacobians [B][N][n][.], ref: the statement at LC.parity_weights in float64 and longdouble), once"""
    if (n, m) not in _INPUTS:
        _, _, Am, Bm = RC.chain_jacobians(n, m, _batch(n))
        _INPUTS[(n, m)] = dict(A=Am, B=Bm, ref=LC.reference(Am, Bm, *LC.parity_weights(n, m)))
    return _INPUTS[(n, m)]


def run_lqr(lib, n, m, Am, Bm, Q, R, Qf):
    """one launch of k_lqr_recur<n, m> -> K [B][N][m][n], P [B][N + 1][n][n], fail [B]; the padding is checked here"""
    B = Am.shape[0]
    Bp = RC.padded(B)
    AB, Wt = RC.pack_AB(Am, Bm, Bp), RC.pack_weights(Q, R, Qf)
    Kt, Pt = np.full((N, n, m, Bp), CANARY), np.full((N + 1, n, n, Bp), CANARY)
    fail = np.full(Bp, int(CANARY), dtype=np.int32)
    assert np.isnan(AB[..., B:]).all() and np.isfinite(AB[..., :B]).all()
    status = lib.recur_lqr(n, m, _ptr(AB), _ptr(Wt), _ptr(Kt), _ptr(Pt), _ptr(fail), B, Bp, N)
    assert status == 0, f"recur_lqr<{n}, {m}>: status {status}"
    for name, out in (("Kt", Kt), ("Pt", Pt), ("fail", fail)):
        assert (out[..., B:] == CANARY).all(), f"{name}: a column b >= B was written"
        assert (out[..., :B] != CANARY).all(), f"{name}: an element of an instance b < B was not written"
    return dict(K=RC.unpack_K(Kt, B), P=RC.unpack_P(Pt, B), fail=fail[:B].copy())


def _lqr_against_the_statement(lib, n, m, c, key):
    Q, R, Qf = LC.parity_weights(n, m)
    got = run_lqr(lib, n, m, c["A"], c["B"], Q, R, Qf)
    assert np.isfinite(got["K"]).all() and np.isfinite(got["P"]).all()
    fr = {}
    try:
        LC.parity(key, c["ref"], got, N, n, m, fr)
    finally:
        RC.record(key, fr[key])
    assert (got["P"] == np.swapaxes(got["P"], 2, 3)).all()
    return got


# ---- the LQR recursion ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m", SHAPES, ids=_ids(SHAPES))
def test_lqr_recur(driver, n, m):
    """parity at LC.parity_weights, then the mixed-failure Qf of tests/test_recur_shapes_gpu.py searched on these inputs"""
    c = inputs(n, m)
    _lqr_against_the_statement(driver, n, m, c, f"k_lqr_recur {n}_{m}")
    Q, R, _ = LC.parity_weights(n, m)
    Qf, K, Pm, fail = RC.mixed_failure(c["A"], c["B"], Q, R, n, f"{n}_{m}")
    RC.check_failure(run_lqr(driver, n, m, c["A"], c["B"], Q, R, Qf), K, Pm, fail)


# ---- the covariance recursion ------------------------------------------------------------------------------------------------------
def run_cov(lib, n, m, F, K, Sigma0, W, w_mode, want):
    """one launch of k_cov_recur<n, m> with F [B][N][n][n], K [B][N][m][n]; Sigma0 None or [B][n][n], W by w_mode"""
    B = F.shape[0]
    Bp = RC.padded(B)
    rows = Bp  # the instance-major arrays have Bp rows too: NaN behind B in the inputs, canaries in the outputs

    def per_instance(a):
        out = np.full((rows,) + a.shape[1:], np.nan)
        out[:B] = a
        return out
    Fp, Kw = RC.instance_fastest(F, Bp, np.nan), RC.instance_fastest(K, Bp, np.nan)
    S0 = None if Sigma0 is None else per_instance(Sigma0)
    Wp = per_instance(W) if w_mode & 1 else np.ascontiguousarray(W, dtype=np.float64)
    shapes = dict(Sigma=(rows, N + 1, n, n), sx=(rows, N + 1, n), su=(rows, N, m), rpos=(rows, N + 1))
    out = {k: np.full(shapes[k], CANARY) for k in want}
    status = lib.recur_cov(n, m, _ptr(Fp), _ptr(Kw), _ptr(S0), 0 if S0 is None else 1, _ptr(Wp), w_mode,
                           *(_ptr(out.get(k)) for k in ("Sigma", "sx", "su", "rpos")), B, Bp, N, rows)
    assert status == 0, f"recur_cov<{n}, {m}>: status {status}"
    for k, v in out.items():
        assert (v[B:] == CANARY).all(), f"{k}: a row b >= B was written"
        assert np.isfinite(v[:B]).all() and (v[:B] != CANARY).all(), f"{k}: NaN or an unwritten element in an instance b < B"
    return {k: np.ascontiguousarray(v[:B]) for k, v in out.items()}


@pytest.mark.parametrize("n,m", SHAPES, ids=_ids(SHAPES))
def test_cov_recur(driver, n, m):
    """F = A + B K with the statement's K; W per instance and knot with Sigma0 per instance, then one W with Sigma0 NULL"""
    c = inputs(n, m)
    B, K = c["A"].shape[0], c["ref"]["K"]
    F = c["A"] + c["B"] @ K
    Sigma0, W = _inputs(B, n, N, 200 + 10 * n + m)
    want = ("Sigma", "sx", "su", "rpos")
    for tag, S0, Wk, w_mode in (("w_mode 3, Sigma0 per instance", Sigma0, W, 3), ("w_mode 0, Sigma0 NULL", None, W[0, 0], 0)):
        got = run_cov(driver, n, m, F, K, S0, Wk, w_mode, want)
        fr = cov_check(f"k_cov_recur {n}_{m} {tag}", got, dict(A=c["A"], B=c["B"], K=K), N, S0, Wk, w_mode, N, n)
        RC.record(f"k_cov_recur {n}_{m}", fr)
        assert (got["Sigma"] == np.swapaxes(got["Sigma"], 2, 3)).all()


# ---- the driver at a shape a plug-in reaches ---------------------------------------------------------------------------------------
def test_lqr_recur_at_a_plugin_shape(A, hip_make, driver):
    """(13, 2) on the oracle's Jacobians of tests/test_recur_shapes_gpu.py's case, against the statement (not against
    altro_lqr_gains): the driver's launch and layouts are the engine's."""
    from test_recur_shapes_gpu import case
    n, m = 13, 2
    c = case(A, hip_make, n, m)
    _lqr_against_the_statement(driver, n, m, c, f"k_lqr_recur {n}_{m}")
