"""Multi-start entry points (include/altro_multistart.h), the parts that need no GPU: the header and the exports, and
everything that is refused before any device work."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS_FUNCTIONS = ("altro_multistart_select", "altro_multistart_select_device", "altro_multistart_spread",
                "altro_multistart_spread_device", "altro_multistart_perturb", "altro_multistart_perturb_device",
                "altro_multistart_get_best", "altro_multistart_get_best_device", "altro_mpc_run_multistart")
MS_METHODS = ("multistart_select", "multistart_select_device", "multistart_spread", "multistart_spread_device", "multistart_perturb",
              "multistart_perturb_device", "multistart_get_best", "multistart_get_best_device", "mpc_run_multistart")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def test_header_and_exports(A):
    """include/altro_multistart.h declares the entry points, the library exports them, and include/altro_hip.h declares none
    of them (every function of that header needs a twin in the oracle)."""
    ms, hip = _declared("altro_multistart.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in MS_FUNCTIONS:
        assert f in ms and f not in hip and hasattr(lib, f), f
    assert sorted(ms) == sorted(MS_FUNCTIONS)
    for method in MS_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("SelectStarts", "SpreadBestStart", "PerturbControls", "GetBestStarts"):
        assert re.search(r"\bvoid %s\(" % name, facade), name


def test_argument_validation_without_a_device(A, P):
    N, B = 20, 6
    s = P.unicycle_turn90(_make(A), batch=B, N=N)
    lib = A.load_library()
    dU = np.zeros((B, N, 2))
    # starts < 1, or not a divisor of the batch: refused whatever else the call carries
    for bad in (0, -1, 4, 5, 7, 12):
        for call in (lambda: s.multistart_select(bad), lambda: s.multistart_spread(bad), lambda: s.multistart_get_best(bad),
                     lambda: s.multistart_perturb_device(bad, 0, 0), lambda: s.multistart_select_device(bad, 0),
                     lambda: s.multistart_spread_device(bad), lambda: s.multistart_get_best_device(bad),
                     lambda: s.mpc_run_multistart(bad, 2, 5)):
            with pytest.raises(A.AltroError) as e:
                call()
            assert f"({A.INVALID_ARG})" in str(e.value) and "starts" in str(e.value), (bad, str(e.value))
    for f in MS_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    # a NULL handle, through raw ctypes
    null = ctypes.c_void_p(None)
    win = (ctypes.c_int * B)()
    buf = (ctypes.c_double * (B * N * 2))()
    assert lib.altro_multistart_select(null, 2, win) == A.INVALID_ARG
    assert lib.altro_multistart_select_device(null, 2, win) == A.INVALID_ARG
    assert lib.altro_multistart_spread(null, 2, win) == A.INVALID_ARG
    assert lib.altro_multistart_spread_device(null, 2, None) == A.INVALID_ARG
    assert lib.altro_multistart_perturb(null, 2, buf, 0) == A.INVALID_ARG
    assert lib.altro_multistart_perturb_device(null, 2, buf, 0) == A.INVALID_ARG
    assert lib.altro_multistart_get_best(null, 2, None, None, None, win) == A.INVALID_ARG
    assert lib.altro_multistart_get_best_device(null, 2, None, None, None, win) == A.INVALID_ARG
    assert lib.altro_mpc_run_multistart(null, 2, 1, 1, None, None, 0, None, None, None, None, None) == A.INVALID_ARG
    # a required pointer NULL (perturb needs no solve, so it is the pointer that is refused)
    assert lib.altro_multistart_perturb(s._h, 2, None, 0) == A.INVALID_ARG
    assert lib.altro_multistart_perturb_device(s._h, 2, None, 1) == A.INVALID_ARG
    # no solve has finished on the handle yet: select, spread and get_best answer NOT_READY, also with starts = 1
    for G in (1, 2, 3, 6):
        for call in (lambda: s.multistart_select(G), lambda: s.multistart_spread(G), lambda: s.multistart_get_best(G),
                     lambda: s.multistart_select_device(G, 0), lambda: s.multistart_spread_device(G),
                     lambda: s.multistart_get_best_device(G)):
            with pytest.raises(A.AltroError) as e:
                call()
            assert f"({A.NOT_READY})" in str(e.value) and "solve" in str(e.value), str(e.value)
    # the loop refuses what the advance refuses, and a loop without a cycle
    for bad_shift in (0, N, -3):
        with pytest.raises(A.AltroError) as e:
            s.mpc_run_multistart(2, 2, bad_shift)
        assert f"({A.INVALID_ARG})" in str(e.value) and "shift" in str(e.value)
    with pytest.raises(A.AltroError) as e:
        s.mpc_run_multistart(2, 0, 5)
    assert f"({A.INVALID_ARG})" in str(e.value)
    t = P.unicycle_turn90(_make(A), batch=B, N=N)
    t.set_steps(np.full(N, 0.1, dtype=np.float32))
    with pytest.raises(A.AltroError) as e:
        t.mpc_run_multistart(2, 2, 5)
    assert f"({A.UNSUPPORTED})" in str(e.value)
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.multistart_perturb(2, np.zeros((3, N, 2)))
    with pytest.raises(ValueError):
        s.mpc_run_multistart(2, 2, 5, w=np.zeros((2, B, 2)))
    with pytest.raises(ValueError):
        s.mpc_run_multistart(2, 2, 5, dU=dU[:, :5])


def test_no_cpu_fallback(A, P):
    """Without a GPU the calls that reach the engine fail with a HIP error -- nothing of multi-start succeeds on the host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_multistart_gpu.py covers the other side
    N, B = 20, 6
    s = P.unicycle_turn90(_make(A), batch=B, N=N)
    for call in (lambda: s.multistart_perturb(2, np.zeros((2, N, 2))), lambda: s.multistart_perturb(3, np.zeros((B, N, 2))),
                 lambda: s.mpc_run_multistart(2, 2, 5), lambda: s.mpc_run_multistart(3, 1, 1, dU=np.zeros((3, N, 2)))):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
    with pytest.raises(A.AltroError):  # (and the solve that select would need cannot run either)
        s.solve()
    with pytest.raises(A.AltroError) as e:
        s.multistart_select(2)
    assert f"({A.NOT_READY})" in str(e.value)
