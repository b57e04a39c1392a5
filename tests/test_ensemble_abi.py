"""Monte-Carlo ensembles (include/altro_ensemble.h), the parts that need no GPU: the generator against its known answers, the
header altro_rng.hpp as a host program under the sanitizers against the numpy statement of tests/_ensemble_common.py, the
public header as C, the exports, everything that is refused before any device work, and the slab rule and staged layouts
against plain loops."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _ensemble_common as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
ENS_FUNCTIONS = ("altro_mpc_ensemble", "altro_mpc_ensemble_device", "altro_noise_fill", "altro_noise_fill_device",
                 "altro_multistart_perturb_gaussian")
ENS_METHODS = ("mpc_ensemble", "mpc_ensemble_device", "noise_fill", "noise_fill_device", "multistart_perturb_gaussian")
N = 12


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for ctr, key, want in EC.KNOWN_ANSWERS:
        got = tuple(int(w) for w in EC.philox(*ctr, *key))
        assert got == want, ([hex(g) for g in got], [hex(w) for w in want])
    # over arrays: the same words as one call at a time
    k = np.arange(5)
    many = EC.philox(k, 7, 1, 3, 11, 13)
    for i in range(5):
        assert tuple(int(w[i]) for w in many) == tuple(int(w) for w in EC.philox(i, 7, 1, 3, 11, 13))


def test_uniforms_are_positive_and_normals_look_normal():
    """u > 0 for the smallest words (the logarithm is finite) and u <= 1 for the largest; 20000 normals of one stream have
    the moments of a standard normal within five standard deviations of the sample moment."""
    assert EC.uniform53(np.uint64(0), np.uint64(0)) == 2.0 ** -54
    assert EC.uniform53(np.uint64(EC.MASK), np.uint64(EC.MASK)) <= 1.0
    z = EC.normals(20261020, np.arange(100)[None, :], np.arange(100)[:, None], 3, EC.STREAM_NOISE, 2).ravel()
    assert z.size == 20000 and np.isfinite(z).all()
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs((z * z).mean() - 1.0) < 5 * np.sqrt(2.0 / z.size)


# ---- 2. altro_rng.hpp as a host program under the sanitizers ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rng_check") / "rng_check"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-ffp-contract=off", "-I" + CSRC, "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "rng_check.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout)


def _fl(v):
    return np.array([float.fromhex(x) for x in v])


def test_host_program_words_and_normals(host):
    assert [tuple(w) for w in host["philox"]] == [want for _, _, want in EC.KNOWN_ANSWERS]
    assert len(host["draws"]) >= 6
    for d in host["draws"]:
        seed, k, s, inst, stream, j = d["in"]
        words = tuple(int(w) for w in EC.draw_words(seed, k, s, inst, stream, j))
        assert words == tuple(d["words"]), d["in"]
        u = (EC.uniform53(np.uint64(words[0]), np.uint64(words[1])), EC.uniform53(np.uint64(words[2]), np.uint64(words[3])))
        assert tuple(_fl(d["u"])) == u and 0.0 < u[0] <= 1.0, d["in"]  # bit for bit
        z = EC.normal_pair(seed, k, s, inst, stream, j)
        err = np.abs(_fl(d["z"]) - np.array([float(z[0]), float(z[1])])).max()
        assert err <= 1e-12, (d["in"], err)
        assert np.abs(_fl(d["z"])).max() < 8.6


def test_host_program_factors(host):
    """Factors of exactly representable matrices equal numpy's bit for bit; the singular ones are factored with zero columns,
    the indefinite ones refused; garbage above the diagonal changes nothing."""
    seen = dict(refused=0, zero_column=0)
    for c in host["factors"]:
        n = c["n"]
        W, L = _fl(c["W"]).reshape(n, n), _fl(c["L"]).reshape(n, n)
        want = EC.psd_factor(W)
        assert (want is None) == bool(c["refused"]), c
        if want is None:
            seen["refused"] += 1
            continue
        assert np.array_equal(L, want), (W, L, want)
        assert np.array_equal(L, np.tril(L)) and np.array_equal(L @ L.T, EC.CC.lower_sym(W))  # (exact for these inputs)
        seen["zero_column"] += int(((L == 0).all(axis=0)).any() and W.any())
        assert np.array_equal(EC.psd_factor(W + np.triu(np.ones((n, n)), 1) * 3.0), want)
    assert seen["refused"] >= 2 and seen["zero_column"] >= 2
    nz = host["noise"]
    seed, k, s, inst = nz["in"]
    xi = EC.normals(seed, k, s, inst, EC.STREAM_NOISE, 4)
    assert np.abs(_fl(nz["xi"]) - xi).max() <= 1e-12
    L = EC.psd_factor(_fl(host["factors"][-1]["W"]).reshape(4, 4))
    assert np.abs(_fl(nz["out"]) - L @ xi).max() <= 1e-12 * np.abs(L).max()
    # the host program's own L xi from its own xi: the fma chain is exact for these integer factors up to one rounding per term
    assert np.abs(_fl(nz["out"]) - L @ _fl(nz["xi"])).max() <= 4 * 2.0 ** -52 * np.abs(L).max() * np.abs(_fl(nz["xi"])).max()


# ---- 5. the slab rule and the staged layouts -------------------------------------------------------------------------------------
def test_slab_rule_and_layouts(host):
    assert host["values"] == [9, 27, 90] and host["stats_doubles"] == 7
    assert len(host["slabs"]) >= 12
    for B, S, slabs, per in host["slabs"]:
        assert (slabs, per) == EC.slabs(B, S), (B, S)
        chunks = -(-S // 64)
        # every chunk belongs to exactly one slab, no slab is empty, and B alone filling the device means one slab
        owner = [c // per for c in range(chunks)]
        assert sorted(set(owner)) == list(range(slabs)) and 1 <= slabs <= 16
        assert slabs == 1 or B < 1024
    # Sigma0: 5 9 | W: 5 2 9 | bounds: 2 2 | mean: 5 3 3 | mom2: 5 3 9 | alive, viol_count: ceil(15 / 2) | summary: 5 7 | stats: 5 7 5
    p = host["ensemble_stage"]
    assert p["cnt"] == [45, 90, 4, 45, 135, 8, 8, 35, 175]
    assert p["off"] == [sum(p["cnt"][:i]) for i in range(10)] and p["total"] == 545
    p = host["ensemble_stage_sparse"]  # one W per knot: 2 9 | alive | stats
    assert p["cnt"] == [0, 18, 0, 0, 0, 8, 0, 0, 175] and p["total"] == 201
    p = host["noise_stage"]  # Sigma0 | W | dx0: 5 7 3 | w: 5 7 2 3
    assert p["cnt"] == [45, 90, 105, 210] and p["off"] == [0, 45, 135, 240, 450]
    assert host["noise_stage_sparse"]["cnt"] == [0, 18, 0, 210]
    assert host["gauss_stage"]["cnt"] == [2]


# ---- 3. the header ----------------------------------------------------------------------------------------------------------------
def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "ens.c"
    src.write_text('#include "altro_ensemble.h"\nint size(void) { return (int)sizeof(altro_ensemble_stats); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_ensemble.h declares the entry points and nothing else, the library exports them, include/altro_hip.h (which
    the oracle mirrors function by function) declares none, and the binding and the facade have their calls."""
    ens, hip = _declared("altro_ensemble.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in ENS_FUNCTIONS:
        assert f in ens and f not in hip and hasattr(lib, f), f
    assert sorted(ens) == sorted(ENS_FUNCTIONS)
    for method in ENS_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    assert A.ENSEMBLE_STATS_DTYPE.itemsize == 56 and A.ENSEMBLE_STATS_DTYPE.names[:4] == ("samples", "stopped_state", "stopped_control", "violated")
    mean, mom2 = np.array([[1.0, 2.0]]), np.array([[[5.0, 2.0], [2.0, 9.0]]])
    assert np.array_equal(A.ensemble_covariance(mean, mom2), np.array([[[4.0, 0.0], [0.0, 5.0]]]))
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("TrackEnsemble", "FillNoise", "PerturbControlsGaussian"):
        assert re.search(r"\b%s\(" % name, facade), name
    # user-model plugins are rebuilt when the generator changes, and find it
    capi = open(os.path.join(CSRC, "altro_capi.cpp")).read()
    assert re.search(r'"altro_devmem\.hpp"[^}]*"altro_rng\.hpp"', capi)
    assert "altro_rng.hpp" in open(os.path.join(CSRC, "Makefile")).read()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device(A, P):
    B, S = 3, 5
    s = P.unicycle_turn90(_make(A), batch=B, N=N)
    lib = A.load_library()
    for f in ENS_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    dbl, ull = ctypes.c_double, ctypes.c_ulonglong
    n, m = 3, 2
    S0 = (dbl * (n * n))(*np.eye(n).ravel())
    mean = (dbl * (B * (N + 1) * n))()
    lo, hi = (dbl * m)(-1.0, -1.0), (dbl * m)(1.0, 1.0)
    dx0 = (dbl * (B * S * n))()
    h = s._h

    def refused(status, got, word=None):
        assert got == status, (got, s._errmsg(h))
        msg = s._errmsg(h)
        assert msg, "altro_last_error is empty"
        assert word is None or word in msg, msg

    def ensemble(steps=N, samples=S, w_mode=0, u_lo=None, u_hi=None, viol_tol=0.0, outs=(mean, None, None, None, None, None), handle=h):
        args = (handle, steps, samples, ull(1), ull(0), S0, 0, None, w_mode, u_lo, u_hi, dbl(viol_tol)) + tuple(outs)
        return [lib.altro_mpc_ensemble(*args), lib.altro_mpc_ensemble_device(*args)]

    def fill(steps=N, samples=S, w_mode=0, outs=(dx0, None), handle=h):
        args = (handle, steps, samples, ull(1), ull(0), S0, 0, None, w_mode) + tuple(outs)
        return [lib.altro_noise_fill(*args), lib.altro_noise_fill_device(*args)]

    def gauss(starts=1, sigma=(0.1, 0.1), handle=h):
        sg = None if sigma is None else (dbl * m)(*sigma)
        return [lib.altro_multistart_perturb_gaussian(handle, starts, ull(1), ull(0), sg, 1)]

    for bad in (0, -1, N + 1):
        for st in ensemble(steps=bad) + fill(steps=bad):
            refused(A.INVALID_ARG, st, "steps")
    for bad in (0, -3):
        for st in ensemble(samples=bad) + fill(samples=bad):
            refused(A.INVALID_ARG, st, "sample")
    for bad in (-1, 4, 7):
        for st in ensemble(w_mode=bad) + fill(w_mode=bad):
            refused(A.INVALID_ARG, st, "w_mode")
    for st in ensemble(u_lo=lo) + ensemble(u_hi=hi):
        refused(A.INVALID_ARG, st, "u_lo")
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        for st in ensemble(viol_tol=bad):
            refused(A.INVALID_ARG, st, "viol_tol")
    for st in ensemble(outs=(None,) * 6) + fill(outs=(None, None)):
        refused(A.INVALID_ARG, st)
    # no backward pass has left gains on the handle (every argument valid)
    for st in ensemble() + ensemble(u_lo=lo, u_hi=hi, w_mode=3):
        refused(A.NOT_READY, st, "gains")
    # sigma: NULL, negative, not finite; starts as altro_multistart_perturb refuses it
    for bad in (None, (-0.1, 0.1), (0.1, float("nan")), (float("inf"), 0.1)):
        for st in gauss(sigma=bad):
            refused(A.INVALID_ARG, st, "sigma")
    for bad in (0, -1, 2, B + 1):
        for st in gauss(starts=bad):
            refused(A.INVALID_ARG, st, "starts")
    # more than 32 states
    big = A.BatchSolver(33, 1, N, B, A.F64)
    S33, out33 = (dbl * (33 * 33))(), (dbl * (B * S * 33))()
    assert lib.altro_noise_fill(big._h, N, S, ull(1), ull(0), S33, 0, None, 0, out33, None) == A.UNSUPPORTED
    assert "32" in big._errmsg(big._h)
    assert lib.altro_mpc_ensemble(big._h, N, S, ull(1), ull(0), S33, 0, None, 0, None, None, dbl(0.0), out33, None, None, None, None,
                                  None) == A.UNSUPPORTED and big._errmsg(big._h)
    big.close()
    # a NULL handle
    null = ctypes.c_void_p(None)
    assert ensemble(handle=null) == [A.INVALID_ARG] * 2 and fill(handle=null) == [A.INVALID_ARG] * 2 and gauss(handle=null) == [A.INVALID_ARG]
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.mpc_ensemble(N, S, Sigma0=np.zeros((2, 2)))
    with pytest.raises(ValueError):
        s.mpc_ensemble(N, S, want=("dev_mean", "median"))
    with pytest.raises(ValueError):
        s.noise_fill(N, S, W=np.zeros((N + 1, 3, 3)))
    with pytest.raises(ValueError):
        s.multistart_perturb_gaussian(1, 1, np.zeros(3))
    s.close()


def test_no_cpu_fallback(A, P):
    """Without a GPU a call that reaches the engine fails with a HIP error: nothing is drawn on the host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_ensemble_gpu.py covers the other side
    s = P.unicycle_turn90(_make(A), batch=3, N=N)
    for call in (lambda: s.noise_fill(N, 4, seed=1, Sigma0=np.eye(3)), lambda: s.multistart_perturb_gaussian(1, 1, np.ones(2))):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
    s.close()


# ---- 10 (CPU side). the purpose test's numpy statement alone stays inside its bar -------------------------------------------------
def test_purpose_bar_holds_for_the_numpy_statement(A, P, oracle_make):
    """The triple integrator of tests/test_ensemble_gpu.py's purpose test on the CPU oracle: its gains and its (exact, linear)
    expansions give Sigma_k by tests/_cov_common.py; the samples of seed 20261020 propagated in numpy through e+ = F e + w give
    the sample second moment, which must stay within 5 sqrt(2 / S) max diag Sigma_k of Sigma_k at every knot."""
    B, S, seed = EC.PURPOSE_B, EC.PURPOSE_S, EC.PURPOSE_SEED
    o = P.triple_integrator(oracle_make, batch=B, N=N)
    o.solve_ilqr()
    K = o.get_gains()[0]
    o.update_expansions()
    ex = [o.get_expansion(k) for k in range(N)]
    o.close()
    Am, Bm = np.stack([e["A"] for e in ex], axis=1), np.stack([e["B"] for e in ex], axis=1)
    Sigma = EC.CC.propagate(Am, Bm, K, N, EC.PURPOSE_SIGMA0, EC.PURPOSE_W, 0)
    dx0, w, _ = EC.noise_arrays(B, S, N, 6, seed, 0, EC.PURPOSE_SIGMA0, EC.PURPOSE_W, 0)
    e = dx0
    for k in range(N + 1):
        M = np.einsum("bsi,bsj->bij", e, e) / S
        bar = 5.0 * np.sqrt(2.0 / S) * np.diagonal(Sigma[:, k], axis1=1, axis2=2).max(axis=1)
        err = np.abs(M - Sigma[:, k]).max(axis=(1, 2))
        assert (err <= bar).all(), (k, err, bar)
        if k < N:
            F = Am[:, k] + Bm[:, k] @ K[:, k]
            e = np.einsum("bij,bsj->bsi", F, e) + w[:, :, k]
