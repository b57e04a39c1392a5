"""Team entry points (include/altro_team.h), the parts that need no GPU: the header as C, the exports, everything that is
refused before any device work, the ring scenario's formulas, and the numpy statements of tests/_team_common.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _team_common as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEAM_FUNCTIONS = ("altro_team_fill_tracks", "altro_team_clearance", "altro_team_clearance_device", "altro_team_solve",
                  "altro_mpc_run_team")
TEAM_METHODS = ("team_fill_tracks", "team_clearance", "team_clearance_device", "team_solve", "mpc_run_team")
N = 12


def _declared(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return set(re.findall(r"\b(altro_[a-z0-9_]+)\s*\(", src))


def _make(A):
    return lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "team.c"
    src.write_text('#include "altro_team.h"\nint modes(void) { return ALTRO_TEAM_ALL + ALTRO_TEAM_PRIORITY; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_team.h declares the five entry points, the library exports them, include/altro_hip.h (which the oracle
    mirrors function by function) declares none, and the binding and the facade have their calls."""
    team, hip = _declared("altro_team.h"), _declared("altro_hip.h")
    lib = A.load_library()
    for f in TEAM_FUNCTIONS:
        assert f in team and f not in hip and hasattr(lib, f), f
    assert sorted(team - {"altro_add_knot_constraint"}) == sorted(TEAM_FUNCTIONS)  # (the header's comment shows that call)
    for method in TEAM_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    assert (A.TEAM_ALL, A.TEAM_PRIORITY) == (0, 1)
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("FillTeamTracks", "TeamClearance", "SolveTeam"):
        assert re.search(r"\b%s\(" % name, facade), name


def test_ring_scenario_is_the_stated_one(P):
    x0, xf = P.team_ring_states(3, 4)
    for t in range(3):
        for a in range(4):
            phi = 2 * np.pi * a / 4 + 0.1 * t
            g = phi + np.pi + 0.2 + 0.05 * t
            assert np.allclose(x0[t * 4 + a], [np.cos(phi), np.sin(phi), phi + np.pi], rtol=0, atol=1e-15)
            assert np.allclose(xf[t * 4 + a], [np.cos(g), np.sin(g), phi + np.pi], rtol=0, atol=1e-15)


def test_numpy_statements():
    """fill_rows, blend_rows, window and clearance of tests/_team_common.py against plain loops."""
    rng = np.random.RandomState(3)
    T, A, K = 2, 4, 5
    X = rng.randn(T * A, K, 3)
    rad = 0.1 + 0.05 * np.arange(T * A)
    for mode in (TC.ALL, TC.PRIORITY):
        rows = TC.fill_rows(X, A, rad, mode)
        for b in range(T * A):
            t, a = divmod(b, A)
            peers = [j for j in range(A) if j != a]
            for i, j in enumerate(peers):
                assert (rows[b, :, 3 * i] == X[t * A + j, :, 0]).all() and (rows[b, :, 3 * i + 1] == X[t * A + j, :, 1]).all()
                want = 0.0 if mode == TC.PRIORITY and j > a else rad[b] + rad[t * A + j]
                assert (rows[b, :, 3 * i + 2] == want).all()
    shared = TC.fill_rows(X, A, rad[:A])
    assert (shared[A:, :, 2] == shared[:A, :, 2]).all()
    old, new = TC.fill_rows(X, A, rad), TC.fill_rows(X + 0.3, A, rad)
    mix = TC.blend_rows(old, new, 0.5)
    assert mix[1, 2, 3] == old[1, 2, 3] + 0.5 * (new[1, 2, 3] - old[1, 2, 3]) and (mix[:, :, 2::3] == new[:, :, 2::3]).all()
    assert (TC.window(old, 3)[:, :, :] == old[:, [3, 4, 4, 4, 4]]).all()
    cl = TC.clearance(X, A, rad, 1, K)
    for t in range(T):
        want = min((X[t * A + a, k, 0] - X[t * A + j, k, 0]) ** 2 + (X[t * A + a, k, 1] - X[t * A + j, k, 1]) ** 2
                   - (rad[t * A + a] + rad[t * A + j]) ** 2 for k in range(1, K) for a in range(A) for j in range(a + 1, A))
        assert abs(cl[t] - want) < 1e-14


def test_refusals_without_a_device(A, P):
    T, Ag = 3, 2
    B = T * Ag
    s = P.team_ring(_make(A), T, Ag, N=N)
    rad, idx = s.team_radius, s.team_circle
    lib = A.load_library()
    for f in TEAM_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    r2 = (ctypes.c_double * 2)(0.15, 0.15)
    out = (ctypes.c_double * B)()
    dbl = ctypes.c_double

    def calls(agents, index, radius, per=0, mode=0, blend=1.0, rounds=1, cycles=1, shift=1):
        h = s._h
        return [lib.altro_team_fill_tracks(h, agents, index, radius, per, mode, dbl(blend)),
                lib.altro_team_solve(h, agents, index, radius, per, mode, dbl(blend), rounds),
                lib.altro_mpc_run_team(h, agents, index, radius, per, mode, dbl(blend), rounds, cycles, shift, None, None, None, None,
                                       None, None),
                lib.altro_team_clearance(h, agents, index, radius, per, out),
                lib.altro_team_clearance_device(h, agents, index, radius, per, out)]
    # agents < 2, or not a divisor of the batch
    for bad in (1, 0, -2, 4, 5, 12):
        assert calls(bad, idx, r2) == [A.INVALID_ARG] * 5, bad
        assert "agents" in s._errmsg(s._h)
    # index: out of range, an ordinary constraint (the control bound, index 0), a knot constraint that is no circle, a circle
    # with the wrong number of parameters
    bound = s.add_knot_constraint(A.CON_CONTROL_BOUND, 0, N, 4)
    wide = s.add_knot_constraint(A.CON_CIRCLE, 1, N, 6)
    for bad in (-1, 99, 0, bound, wide):
        assert calls(Ag, bad, r2) == [A.INVALID_ARG] * 5, bad
    # mode, blend, rounds, cycles: the calls that take them
    for kw in (dict(mode=2), dict(mode=-1), dict(blend=0.0), dict(blend=-0.5), dict(blend=1.5), dict(blend=float("nan")),
               dict(blend=float("inf"))):
        assert calls(Ag, idx, r2, **kw)[:3] == [A.INVALID_ARG] * 3, kw
    assert calls(Ag, idx, r2, rounds=0)[1:3] == [A.INVALID_ARG] * 2
    assert calls(Ag, idx, r2, cycles=0)[2] == A.INVALID_ARG
    # radius: NULL, negative, not finite -- shared and per instance
    assert calls(Ag, idx, None) == [A.INVALID_ARG] * 5
    for bad in (-0.1, float("nan"), float("inf")):
        assert calls(Ag, idx, (ctypes.c_double * 2)(0.15, bad)) == [A.INVALID_ARG] * 5, bad
        per = (ctypes.c_double * B)(*([0.15] * (B - 1) + [bad]))
        assert calls(Ag, idx, per, per=1) == [A.INVALID_ARG] * 5, bad
    # a NULL handle, a NULL clearance output
    null = ctypes.c_void_p(None)
    assert lib.altro_team_fill_tracks(null, Ag, idx, r2, 0, 0, dbl(1.0)) == A.INVALID_ARG
    assert lib.altro_team_clearance(null, Ag, idx, r2, 0, out) == A.INVALID_ARG
    assert lib.altro_team_clearance_device(null, Ag, idx, r2, 0, out) == A.INVALID_ARG
    assert lib.altro_team_solve(null, Ag, idx, r2, 0, 0, dbl(1.0), 1) == A.INVALID_ARG
    assert lib.altro_mpc_run_team(null, Ag, idx, r2, 0, 0, dbl(1.0), 1, 1, 1, None, None, None, None, None, None) == A.INVALID_ARG
    assert lib.altro_team_clearance(s._h, Ag, idx, r2, 0, None) == A.INVALID_ARG
    assert lib.altro_team_clearance_device(s._h, Ag, idx, r2, 0, None) == A.INVALID_ARG
    # the loop refuses what the advance refuses
    for bad_shift in (0, N, -3):
        with pytest.raises(A.AltroError) as e:
            s.mpc_run_team(Ag, idx, rad, cycles=2, shift=bad_shift)
        assert f"({A.INVALID_ARG})" in str(e.value) and "shift" in str(e.value)
    t = P.team_ring(_make(A), T, Ag, N=N)
    t.set_steps(np.full(N, 0.1, dtype=np.float32))
    with pytest.raises(A.AltroError) as e:
        t.mpc_run_team(Ag, t.team_circle, rad, cycles=2, shift=3)
    assert f"({A.UNSUPPORTED})" in str(e.value)
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.team_fill_tracks(Ag, idx, np.zeros(3))
    with pytest.raises(ValueError):
        s.mpc_run_team(Ag, idx, rad, cycles=2, shift=3, w=np.zeros((2, B, 2)))


def test_no_cpu_fallback(A, P):
    """Without a GPU the calls that reach the engine fail with a HIP error -- nothing of the team calls succeeds on the host."""
    r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                       timeout=300)  # (in a child: torch's HIP runtime must not take the device in this process)
    if r.stdout.strip().endswith("True"):
        return  # the error path needs a machine without a device; tests/test_team_gpu.py covers the other side
    s = P.team_ring(_make(A), 3, 2, N=N)
    rad, idx = s.team_radius, s.team_circle
    for call in (lambda: s.team_fill_tracks(2, idx, rad), lambda: s.team_fill_tracks(2, idx, rad, A.TEAM_PRIORITY, 0.5),
                 lambda: s.team_clearance(2, idx, rad), lambda: s.team_clearance_device(2, idx, rad, 8),
                 lambda: s.team_solve(2, idx, rad, rounds=2), lambda: s.mpc_run_team(2, idx, rad, cycles=2, shift=3)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
