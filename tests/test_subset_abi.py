"""The solve mask and sequential team rounds (include/altro_subset.h), the parts that need no GPU: the header as C, the
exports, everything that is refused before any device work, and the numpy statements of tests/_subset_common.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _subset_common as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBSET_FUNCTIONS = ("altro_set_solve_mask", "altro_set_solve_mask_device", "altro_get_solve_mask", "altro_team_solve_sequential")
SUBSET_METHODS = ("set_solve_mask", "set_solve_mask_device", "get_solve_mask", "team_solve_sequential")
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


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "subset.c"
    src.write_text('#include "altro_subset.h"\n'
                   "altro_status clear(altro_handle h) { return altro_set_solve_mask(h, (const unsigned char*)0); }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                        "-fsyntax-only", str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_header_and_exports(A):
    """include/altro_subset.h declares the four entry points and nothing else, the library exports them, include/altro_hip.h
    and include/altro_team.h declare none of them, and the binding and the facade have their calls."""
    sub, hip, team = _declared("altro_subset.h"), _declared("altro_hip.h"), _declared("altro_team.h")
    lib = A.load_library()
    for f in SUBSET_FUNCTIONS:
        assert f in sub and f not in hip and f not in team and hasattr(lib, f), f
    assert sorted(sub) == sorted(SUBSET_FUNCTIONS)
    for method in SUBSET_METHODS:
        assert callable(getattr(A.BatchSolver, method)), method
    facade = open(os.path.join(ROOT, "include", "altro", "altro.hpp")).read()
    for name in ("SetSolveMask", "ClearSolveMask", "GetSolveMask", "SolveTeamSequential"):
        assert re.search(r"\b%s\(" % name, facade), name
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "subset_facade_driver.cpp"))


def test_refusals_without_a_device(A, P):
    T, Ag = 2, 3
    B = T * Ag
    s = P.team_ring(_make(A), T, Ag, N=N)
    lib = A.load_library()
    for f in SUBSET_FUNCTIONS:
        getattr(lib, f).restype = ctypes.c_int
    h, null = s._h, ctypes.c_void_p(None)
    mask = (ctypes.c_ubyte * B)(*([1, 0] * (B // 2)))
    count = ctypes.c_int(-1)
    rad = (ctypes.c_double * Ag)(*([0.15] * Ag))

    def refused(status, got, word=None):
        assert got == status, (got, s._errmsg(h))
        msg = s._errmsg(h)
        assert msg, "altro_last_error is empty"
        assert word is None or word in msg, msg

    # a NULL handle
    assert lib.altro_set_solve_mask(null, mask) == A.INVALID_ARG
    assert lib.altro_set_solve_mask_device(null, mask) == A.INVALID_ARG
    assert lib.altro_get_solve_mask(null, mask, ctypes.byref(count)) == A.INVALID_ARG
    assert lib.altro_team_solve_sequential(null, Ag, s.team_circle, rad, 0, 1) == A.INVALID_ARG
    # a NULL pointer where one is needed
    refused(A.INVALID_ARG, lib.altro_set_solve_mask_device(h, null), "mask_device")
    refused(A.INVALID_ARG, lib.altro_get_solve_mask(h, null, ctypes.byref(count)), "mask")
    # the sequential rounds: what altro_team_solve refuses, with sweeps in place of rounds
    seq = lib.altro_team_solve_sequential
    for bad in (1, 0, -2, 4):  # agents < 2, or not a divisor of the batch
        refused(A.INVALID_ARG, seq(h, bad, s.team_circle, rad, 0, 1), "agents")
    for bad in (-1, 99, 0):  # out of range; constraint 0 is the control bound
        refused(A.INVALID_ARG, seq(h, Ag, bad, rad, 0, 1), "constraint")
    refused(A.INVALID_ARG, seq(h, 2, s.team_circle, rad, 0, 1), "nparams")  # the circle has 3 (3 - 1) parameters, not 3 (2 - 1)
    refused(A.INVALID_ARG, seq(h, Ag, s.team_circle, null, 0, 1), "radius")
    for bad in (-0.1, float("nan"), float("inf")):
        r = (ctypes.c_double * Ag)(0.15, bad, 0.15)
        refused(A.INVALID_ARG, seq(h, Ag, s.team_circle, r, 0, 1), "radius")
    for bad in (0, -3):
        refused(A.INVALID_ARG, seq(h, Ag, s.team_circle, rad, 0, bad), "sweep")
    # shapes the Python layer checks itself
    with pytest.raises(ValueError):
        s.set_solve_mask(np.ones(B + 1))
    with pytest.raises(ValueError):
        s.team_solve_sequential(Ag, s.team_circle, np.zeros(Ag + 1))
    s.close()


def test_no_cpu_fallback(A, P):
    """Without a GPU every call that reaches the engine fails with a HIP error: no mask is kept on the host and nothing is
    solved there."""
    if _has_gpu():
        return  # the error path needs a machine without a device; tests/test_subset_gpu.py covers the other side
    s = P.team_ring(_make(A), 2, 3, N=N)
    for call in (lambda: s.set_solve_mask(np.arange(6) % 2), lambda: s.set_solve_mask(None), lambda: s.set_solve_mask_device(8),
                 lambda: s.get_solve_mask(), lambda: s.team_solve_sequential(3, s.team_circle, s.team_radius, 1)):
        with pytest.raises(A.AltroError) as e:
            call()
        assert f"({A.HIP_ERROR})" in str(e.value) or "hip" in str(e.value).lower()
    s.close()


def test_numpy_statements():
    """The ordered compaction per chain slice against a plain loop; the slices; a full mask gives 0, 1, 2, ...; the count of a
    team's turn."""
    rng = np.random.RandomState(11)
    assert SC.chain_slices(6) == [(0, 6)] and SC.chain_slices(700) == [(0, 700)] and SC.chain_slices(2047) == [(0, 2047)]
    assert SC.chain_slices(2100) == [(0, 576), (576, 1152), (1152, 1728), (1728, 2100)]
    assert SC.chain_slices(4096) == [(0, 1024), (1024, 2048), (2048, 3072), (3072, 4096)]
    assert SC.chain_slices(2049) == [(0, 576), (576, 1152), (1152, 1728), (1728, 2049)]
    assert SC.chain_slices(130, chains=4) == [(0, 64), (64, 128), (128, 130)]  # (a fourth slice would be empty)
    for B in (1, 6, 65, 700, 2100, 4096):
        slices = SC.chain_slices(B)
        assert slices[0][0] == 0 and slices[-1][1] == B and all(a[1] == b[0] for a, b in zip(slices, slices[1:]))
        assert all(hi > lo and (lo % SC.WAVE == 0) for lo, hi in slices)
        for name, mask in list(SC.patterns(B).items()) + [("random", rng.rand(B) < 0.3)]:
            got, counts = SC.compact(mask, slices)
            want, wcounts = SC.compact_loop(mask, slices)
            assert (got == want).all() and (counts == wcounts).all(), (B, name)
            assert counts.sum() == int(np.asarray(mask).sum())
            for c, (lo, hi) in enumerate(slices):
                part = got[lo:lo + counts[c]]
                assert (np.diff(part) > 0).all() and ((part >= lo) & (part < hi)).all() and (got[lo + counts[c]:hi] == -1).all()
        assert (SC.compact(np.ones(B), slices)[0] == np.arange(B)).all()
        for Ag in (2, 3, 5, 8):
            for a in range(Ag):
                turn = np.arange(B) % Ag == a
                for lo, hi in slices:
                    assert SC.turn_count(lo, hi, Ag, a) == int(turn[lo:hi].sum()), (B, Ag, a, lo, hi)
    pats = SC.patterns(2100)
    assert not pats["empty_chain"][:576].any() and pats["empty_chain"][576:].all()
    assert pats["spread40"].sum() == 40 and all(pats["spread40"][lo:hi].any() for lo, hi in SC.chain_slices(2100))
