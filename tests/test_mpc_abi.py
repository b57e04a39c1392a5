"""Receding-horizon entry points (include/altro_mpc.h), the parts that need no GPU: the header and the exports, the
per-constraint row map against a numpy statement of the contract, and argument validation."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _mpc_common as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPC_FUNCTIONS = ("altro_mpc_row_map", "altro_mpc_advance", "altro_mpc_advance_device", "altro_mpc_run",
                 "altro_get_initial_state", "altro_set_penalties")


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def test_header_and_exports(A):
    """include/altro_mpc.h declares the entry points, the library exports them, and include/altro_hip.h declares none of
    them (every function of that header needs a twin in the oracle)."""
    mpc, hip = _declared("altro_mpc.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in MPC_FUNCTIONS:
        assert f in mpc and f not in hip and hasattr(lib, f), f
    assert not [f for f in mpc if not hasattr(lib, f)]
    assert "al_solver.hpp:292-297" in open(os.path.join(ROOT, "include", "altro_mpc.h")).read()
    for method in ("mpc_row_map", "mpc_advance", "mpc_advance_device", "mpc_run", "get_initial_state", "set_penalties"):
        assert callable(getattr(A.BatchSolver, method))


@pytest.mark.parametrize("problem", ["turn90", "three_obstacles", "mixed"])
def test_row_map_is_the_numpy_statement(A, P, problem):
    N = 100
    if problem == "turn90":
        s, cons = P.unicycle_turn90(_make(A), batch=2, N=N), M.TURN90_CONS(N)
    elif problem == "three_obstacles":
        s, cons = P.unicycle_three_obstacles(_make(A), batch=2, N=N, dtype=A.F32), M.THREE_OBSTACLES_CONS(N)
    else:
        s, cons = M.mixed_problem(A, P, _make(A), batch=2), M.MIXED_CONS
    resets = {}
    for shift in (1, 5, 45, N - 1):
        got = s.mpc_row_map(shift)
        want = M.row_map(N, shift, cons)
        assert got.dtype == np.int32 and np.array_equal(got, want), (problem, shift)
        resets[shift] = int((got < 0).sum())
        # a row never comes from in front of itself: what lets the device shift in place, front to back
        assert (got[got >= 0] >= np.nonzero(got >= 0)[0]).all()
    if problem == "mixed":
        assert len(got) == 552 and resets == {1: 1, 5: 5, 45: 45, N - 1: 59}
        # the equality sits in front of the bound on the knots that carry both: rows of knot 70 are goal (3), bound (4)
        labels = M.row_labels(N, cons)
        assert [j for k, j, _ in labels if k == 70] == [2, 2, 2, 0, 0, 0, 0]
        # under a shift of 5 the circle's row at knots 55 .. 59 starts afresh; the bound next to it keeps its source
        assert [labels[r][:2] for r in np.nonzero(s.mpc_row_map(5) < 0)[0]] == [(k, 1) for k in range(55, 60)]
    else:
        assert resets == {1: 0, 5: 0, 45: 0, N - 1: 0}
    if problem == "three_obstacles":
        # knot 0 carries only the bound, knots 1 .. N-1 circles + bound: the bound's duals move from knot `shift` to knot 0
        # although the two knots are of different classes
        labels = M.row_labels(N, cons)
        m5 = s.mpc_row_map(5)
        assert [labels[r] for r in m5[:4]] == [(5, 1, i) for i in range(4)]


def test_mixed_problem_rows_agree_with_the_oracle(A, P, oracle_make):
    o = M.mixed_problem(A, P, oracle_make, batch=1)
    assert o.num_constraints() == 552 == len(M.row_labels(M.MIXED_N, M.MIXED_CONS))
    for k in (0, 1, 59, 60, 69, 70, 99, 100):
        assert o.num_constraints(k) == sum(1 for kk, _, _ in M.row_labels(M.MIXED_N, M.MIXED_CONS) if kk == k)


def test_argument_validation_without_a_device(A, P):
    N = 20
    s = P.unicycle_turn90(_make(A), batch=2, N=N)
    lib = A.load_library()
    for bad in (0, -1, N, N + 7):
        for call in (lambda: s.mpc_row_map(bad), lambda: s.mpc_advance(bad), lambda: s.mpc_advance_device(bad),
                     lambda: s.mpc_run(2, bad)):
            with pytest.raises(A.AltroError) as e:
                call()
            assert f"({A.INVALID_ARG})" in str(e.value) and "shift" in str(e.value)
    with pytest.raises(A.AltroError) as e:
        s.mpc_run(0, 1)
    assert f"({A.INVALID_ARG})" in str(e.value)
    lib.altro_mpc_row_map.restype = lib.altro_get_initial_state.restype = lib.altro_set_penalties.restype = int
    assert lib.altro_mpc_row_map(s._h, 1, None) == A.INVALID_ARG
    assert lib.altro_mpc_row_map(None, 1, None) == A.INVALID_ARG
    assert lib.altro_get_initial_state(s._h, None) == A.INVALID_ARG
    assert lib.altro_set_penalties(s._h, None) == A.INVALID_ARG
    assert len(s.mpc_row_map(N - 1)) == 4 * N + 3
    with pytest.raises(ValueError):
        s.mpc_advance(1, w=np.zeros((3, 3)))
    # per-knot steps, times and models would have to move along the horizon too: refused, not ignored
    t = P.unicycle_turn90(_make(A), batch=2, N=N)
    t.set_steps(np.full(N, 0.1, dtype=np.float32))
    for call in (lambda: t.mpc_row_map(1), lambda: t.mpc_advance(1), lambda: t.mpc_run(2, 1)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.UNSUPPORTED})" in str(e.value)
    t.set_uniform_step(np.float32(0.1))  # (back to one step for the whole horizon)
    assert len(t.mpc_row_map(1)) == 4 * N + 3
    t.set_times(np.arange(N + 1, dtype=np.float32))
    with pytest.raises(A.AltroError) as e:
        t.mpc_advance(1)
    assert f"({A.UNSUPPORTED})" in str(e.value)
    u = A.BatchSolver(3, 2, N, 1)
    u.set_knot_models(np.zeros(N, dtype=np.int32))
    with pytest.raises(A.AltroError) as e:
        u.mpc_row_map(1)
    assert f"({A.UNSUPPORTED})" in str(e.value)


def test_no_cpu_fallback_for_the_advance(A, P):
    """Without a GPU the advance fails with a HIP error -- it never succeeds on the host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_mpc_gpu.py covers the other side
    s = P.unicycle_turn90(_make(A), batch=2, N=20)
    for call in (lambda: s.mpc_advance(1), lambda: s.mpc_advance(1, x0=np.zeros(3), w=np.zeros((2, 3))), lambda: s.mpc_run(2, 1),
                 s.get_initial_state, lambda: s.set_penalties(np.ones((2, 83)))):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
