"""Event-triggered re-planning (include/altro_trigger.h), the parts that need no GPU: the header as C and as C++, the exports,
the layout of altro_trigger_rule against the binding's ctypes struct, and everything that is refused before any device work --
but for the cost-to-go refusal: altro_set_record_ctg itself needs a device, so a handle can carry that flag only where there
is one (tests/test_trigger_gpu.py::test_refusals_on_the_device)."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _trigger_common as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIGGER_FUNCTIONS = ("altro_mpc_trigger", "altro_mpc_trigger_device", "altro_mpc_run_triggered")
TRIGGER_METHODS = ("mpc_trigger", "mpc_trigger_device", "mpc_run_triggered")
FIELDS = ("max_age", "dx_tol", "viol_tol", "on_unsolved", "lookahead", "ahead_tol")
N = 12


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def _has_gpu():
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    return r.stdout.strip().endswith("True")


USE = ('#include "altro_trigger.h"\n'
       "altro_status age_only(altro_handle h, unsigned char* mask) {\n"
       "  altro_trigger_rule r;\n"
       "  r.max_age = 2; r.dx_tol = -1.0; r.viol_tol = -1.0; r.on_unsolved = 0; r.lookahead = 0; r.ahead_tol = 0.0;\n"
       "  return altro_mpc_trigger(h, &r, 0, 0, 0, 0, mask, 0);\n"
       "}\n"
       "int bits(void) { return ALTRO_TRIGGER_FIRST | ALTRO_TRIGGER_AGE | ALTRO_TRIGGER_DEVIATION | ALTRO_TRIGGER_VIOLATION |\n"
       "                        ALTRO_TRIGGER_LIMIT | ALTRO_TRIGGER_UNSOLVED | ALTRO_TRIGGER_AHEAD; }\n")


@pytest.mark.parametrize("compiler,std,ext", [("gcc", "-std=c99", ".c"), ("g++", "-std=c++17", ".cpp")])
def test_header_compiles_as_c_and_as_cxx(tmp_path, compiler, std, ext):
    src = tmp_path / ("trigger" + ext)
    src.write_text(USE)
    r = subprocess.run([compiler, std, "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                        str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_trigger.h declares the three entry points and nothing else, the library exports them, the older headers
    declare none of them, and the binding and the facade have their calls."""
    trig = _declared("altro_trigger.h")
    lib = A.load_library()
    for f in TRIGGER_FUNCTIONS:
        assert f in trig and hasattr(lib, f), f
        for other in ("altro_hip.h", "altro_mpc.h", "altro_subset.h"):
            assert f not in _declared(other), (f, other)
    assert sorted(trig) == sorted(TRIGGER_FUNCTIONS)
    for method in TRIGGER_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("EvaluateTrigger", "RunTriggered"):
        assert re.search(r"\b%s\(" % name, facade), name
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "trigger_facade_driver.cpp"))


def test_rule_layout_matches_the_binding(A, tmp_path):
    """sizeof and offsetof of altro_trigger_rule as a C compiler lays it out, against the ctypes struct"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "altro_trigger.h"\n'
                   "int main(void) {\n"
                   '  printf("%d", (int)sizeof(altro_trigger_rule));\n'
                   + "".join('  printf(" %%d", (int)offsetof(altro_trigger_rule, %s));\n' % f for f in FIELDS)
                   + "  return 0;\n}\n")
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    assert [name for name, _ in A.TriggerRule._fields_] == list(FIELDS)
    assert got == [ctypes.sizeof(A.TriggerRule)] + [getattr(A.TriggerRule, f).offset for f in FIELDS], got
    assert got[0] == 40
    r = A.TriggerRule(max_age=3, dx_tol=1e-3)
    assert (r.max_age, r.dx_tol, r.viol_tol, r.on_unsolved, r.lookahead, r.ahead_tol) == (3, 1e-3, -1.0, 0, 0, 0.0)


def test_refusals_without_a_device(A, P):
    B = 3
    s = P.unicycle_turn90(_make(A), batch=B, N=N)
    lib = A.load_library()
    for f in TRIGGER_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    h, null = s._h, ctypes.c_void_p(None)
    mask = (ctypes.c_ubyte * B)()
    why = (ctypes.c_int * B)()
    lo = (ctypes.c_double * 2)(-1.5, -1.5)
    hi = (ctypes.c_double * 2)(1.5, 1.5)

    def refused(status, got, word=None):
        assert got == status, (got, s._errmsg(h))
        msg = s._errmsg(h)
        assert msg, "altro_last_error is empty"
        assert word is None or word in msg, msg

    def evaluate(rule, u_lo=None, u_hi=None, handle=h):
        r = None if rule is None else ctypes.byref(rule)
        return [lib.altro_mpc_trigger(handle, r, None, None, u_lo, u_hi, mask, why),
                lib.altro_mpc_trigger_device(handle, r, None, None, u_lo, u_hi, mask, why)]

    def run(rule, cycles=2, shift=2, u_lo=None, u_hi=None, handle=h):
        r = None if rule is None else ctypes.byref(rule)
        return [lib.altro_mpc_run_triggered(handle, cycles, shift, None, u_lo, u_hi, r, None, None, None, None, None, why)]

    def both(rule, **kw):
        return evaluate(rule, **kw) + run(rule, **kw)
    ok = A.TriggerRule(max_age=2, dx_tol=1e-3)
    # a NULL handle, a NULL rule
    assert both(ok, handle=null) == [A.INVALID_ARG] * 3
    for st in both(None):
        refused(A.INVALID_ARG, st, "rule")
    # max_age < 1
    for bad in (0, -3):
        for st in both(A.TriggerRule(max_age=bad)):
            refused(A.INVALID_ARG, st, "max_age")
    # a NaN tolerance
    nan = float("nan")
    for rule in (A.TriggerRule(dx_tol=nan), A.TriggerRule(viol_tol=nan), A.TriggerRule(lookahead=2, ahead_tol=nan)):
        for st in both(rule):
            refused(A.INVALID_ARG, st, "NaN")
    # lookahead outside [0, N]
    for bad in (-1, N + 1):
        for st in both(A.TriggerRule(lookahead=bad, ahead_tol=1e-4)):
            refused(A.INVALID_ARG, st, "lookahead")
    # ahead_tol < 0 with a lookahead (and read only with one)
    for st in both(A.TriggerRule(lookahead=2, ahead_tol=-1e-4)):
        refused(A.INVALID_ARG, st, "ahead_tol")
    # exactly one of u_lo / u_hi
    for kw in (dict(u_lo=lo), dict(u_hi=hi)):
        for st in both(ok, **kw):
            refused(A.INVALID_ARG, st, "u_lo")
    # the run: cycles < 1, a shift that altro_mpc_advance refuses, the age bound
    for bad in (0, -1):
        refused(A.INVALID_ARG, run(ok, cycles=bad)[0], "cycle")
    for bad in (0, -1, N, N + 3):
        refused(A.INVALID_ARG, run(ok, shift=bad)[0], "shift")
    refused(A.INVALID_ARG, run(A.TriggerRule(max_age=4), shift=4)[0], "held tail")        # 3 * 4 + 4 = 16 > 12
    refused(A.INVALID_ARG, run(A.TriggerRule(max_age=3, lookahead=5, ahead_tol=0.0), shift=4)[0], "held tail")  # 8 + 5 > 12
    # the lookahead before any gains exist: the evaluation answers NOT_READY (every argument valid)
    for st in evaluate(A.TriggerRule(lookahead=3, ahead_tol=1e-4), u_lo=lo, u_hi=hi):
        refused(A.NOT_READY, st, "gains")
    # per-knot steps do not move along the horizon
    t = P.unicycle_turn90(_make(A), batch=B, N=N)
    t.set_steps(np.full(N, 0.05, dtype=np.float32))
    for st in both(ok, handle=t._h):
        assert st == A.UNSUPPORTED and "per-knot" in t._errmsg(t._h), (st, t._errmsg(t._h))
    t.close()
    # a missing reference path, as altro_mpc_run_tracked answers
    t = P.unicycle_turn90(_make(A), batch=B, N=N, constraints=False)
    t.set_lqr_tracking_cost(0, N + 1, np.ones(3), np.ones(2))
    for st in both(ok, handle=t._h):
        assert st == A.NOT_READY and "reference" in t._errmsg(t._h), (st, t._errmsg(t._h))
    t.close()
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.mpc_trigger(dict(max_age=2), age=np.zeros(B + 1))
    with pytest.raises(ValueError):
        s.mpc_trigger(dict(max_age=2), tracked=np.zeros(B + 1, dtype=A.TRACK_STATS_DTYPE))
    with pytest.raises(ValueError):
        s.mpc_run_triggered(2, 2, dict(max_age=2), w=np.zeros((2, B, N)))
    s.close()


def test_no_cpu_fallback(A, P):
    """A valid call without a device returns ALTRO_HIP_ERROR: no rule is evaluated and nothing is solved on the host."""
    if _has_gpu():
        return  # the error path needs a machine without a device; tests/test_trigger_gpu.py covers the other side
    s = P.unicycle_turn90(_make(A), batch=3, N=N)
    rule = TG.rule_dict(max_age=2, dx_tol=1e-3)
    for call in (lambda: s.mpc_trigger(rule), lambda: s.mpc_trigger(rule, age=np.arange(3)), lambda: s.mpc_trigger_device(rule, mask_ptr=8),
                 lambda: s.mpc_run_triggered(2, 2, rule)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value), str(e.value)
    s.close()
