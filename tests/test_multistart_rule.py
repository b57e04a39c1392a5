"""Host-only: the multi-start selection rule (include/altro_multistart.h; altro-cpp_amd/csrc/altro_common.hpp: ms_select, the
ONE function the kernel k_ms_select calls too).  tests/cpp/multistart_rule_driver.cpp is built with plain g++ and runs the
rule over hand-made keys; the winners are compared with the numpy statement of the rule in tests/_multistart_common.py.
This is where NaN and the infinities are covered: no GPU test feeds the solver a NaN."""
import os
import subprocess

import numpy as np
import pytest

import _multistart_common as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
NAN, INF = float("nan"), float("inf")
S, U, MI = 0, 1, 7  # ALTRO_SOLVED, ALTRO_UNSOLVED, ALTRO_MAX_INNER_ITERATIONS


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    d = tmp_path_factory.mktemp("multistart_rule")
    exe = d / "multistart_rule_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "multistart_rule_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(groups):
        """groups: list of lists of (status, cost, violation), all of one length.  Returns (winners, classes)."""
        keys = np.array(groups, dtype=np.float64)
        assert keys.ndim == 3 and keys.shape[2] == 3
        path = d / "keys.bin"
        keys.tofile(str(path))
        r = subprocess.run([str(exe), str(path), str(keys.shape[0]), str(keys.shape[1])], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        rows = np.array([[int(v) for v in line.split()] for line in r.stdout.splitlines()])
        return rows[:, 0], rows[:, 1:]
    return run


def _numpy(groups):
    k = np.array(groups, dtype=np.float64)
    win = np.array([MS.rule_winner(g[:, 0].astype(int), g[:, 1], g[:, 2]) for g in k])
    cls = np.array([MS.rule_class(g[:, 0].astype(int), g[:, 1], g[:, 2]) for g in k])
    return win, cls


def test_constants_match_the_c_header():
    import re
    src = open(os.path.join(ROOT, "include", "altro_hip.h")).read()
    for name, value in (("ALTRO_SOLVED", S), ("ALTRO_UNSOLVED", U), ("ALTRO_MAX_INNER_ITERATIONS", MI)):
        assert re.search(r"\b%s = %d," % (name, value), src), name
    assert MS.SOLVED == S


def test_every_class_and_its_order(rule):
    groups = [
        [(MI, 1.0, 0.5), (S, 9.0, 1e-7), (S, 8.0, 1e-3), (U, 0.1, 0.0)],        # solved beats unsolved; lowest cost among the solved
        [(MI, 5.0, 0.5), (U, 9.0, 0.25), (MI, 1.0, 0.25), (MI, 0.5, 0.75)],     # no solved start: violation, then cost
        [(MI, NAN, 0.0), (U, 3.0, INF), (MI, 7.0, 9.0), (S, NAN, 0.0)],         # class 2 loses to any finite start
        [(S, NAN, 0.0), (S, 1.0, INF), (MI, -INF, 0.0), (U, 0.0, NAN)],         # all class 2: the start index alone
        [(S, INF, 0.0), (MI, 1.0, 2.0), (S, 2.0, -INF), (MI, 1.0, 1.0)],        # a SOLVED start with a non-finite number is class 2
        [(MI, 2.0, 1.0), (S, 3.0, 0.0), (S, 3.0, 5.0), (S, 3.0, 0.0)],          # class 0 ignores the violation: exact tie -> lowest index
    ]
    win, cls = rule(groups)
    assert win.tolist() == [2, 2, 2, 0, 3, 1]
    assert cls.tolist() == [[1, 0, 0, 1], [1, 1, 1, 1], [2, 2, 1, 2], [2, 2, 2, 2], [2, 1, 2, 1], [1, 0, 0, 0]]
    nwin, ncls = _numpy(groups)
    assert np.array_equal(win, nwin) and np.array_equal(cls, ncls)


def test_exact_ties_and_signed_zero(rule):
    groups = [
        [(S, 0.0, 0.0), (S, -0.0, 0.0), (S, 0.0, 0.0)],       # -0.0 against 0.0: a tie, the lowest index
        [(S, -0.0, 0.0), (S, 0.0, 0.0), (S, -0.0, 0.0)],
        [(MI, 1.0, 0.0), (MI, 1.0, -0.0), (MI, 0.5, 1.0)],    # ... in the violation of class 1 as well
        [(MI, 1.0, -0.0), (MI, 0.5, 0.0), (MI, 0.5, -0.0)],   # tie in the violation, the cost decides, then the index
        [(U, 4.0, 2.0), (MI, 4.0, 2.0), (U, 4.0, 2.0)],       # the status does not order class 1
    ]
    win, _ = rule(groups)
    assert win.tolist() == [0, 0, 0, 1, 0]
    assert np.array_equal(win, _numpy(groups)[0])


def test_one_start(rule):
    groups = [[(S, 1.0, 0.0)], [(MI, 2.0, 3.0)], [(U, NAN, NAN)]]
    win, cls = rule(groups)
    assert win.tolist() == [0, 0, 0] and cls[:, 0].tolist() == [0, 1, 2]


@pytest.mark.parametrize("G", [3, 5, 7, 9, 13])
def test_random_keys_against_numpy(rule, G):
    """A G that is no power of two; costs and violations drawn from a few values, so that ties are the rule, with NaN and
    infinities mixed in.  The winner is also the same whatever order the starts are reduced in: the winner of a rotated group
    is the rotated winner unless an exact tie moves it to the tie's lowest index -- checked through the key, not the index."""
    rng = np.random.default_rng(1234 + G)
    vals = np.array([0.0, -0.0, 0.5, 1.0, 1.0 + 2.0 ** -52, 2.0, NAN, INF, -INF])
    pv = np.array([3, 2, 4, 4, 4, 4, 1, 1, 1], dtype=float)
    groups = np.stack([rng.choice([S, U, MI], size=(200, G)).astype(np.float64), rng.choice(vals, size=(200, G), p=pv / pv.sum()),
                       rng.choice(vals, size=(200, G), p=pv / pv.sum())], axis=2)
    win, cls = rule(groups.tolist())
    nwin, ncls = _numpy(groups)
    assert np.array_equal(cls, ncls)
    assert np.array_equal(win, nwin)
    rot = np.roll(groups, 2, axis=1)
    rwin, _ = rule(rot.tolist())
    for p in range(len(groups)):
        a, b = groups[p, win[p]], rot[p, rwin[p]]
        ca, cb = MS.rule_class([int(a[0])], [a[1]], [a[2]])[0], MS.rule_class([int(b[0])], [b[1]], [b[2]])[0]
        assert ca == cb
        if ca == 0:
            assert a[1] == b[1]
        elif ca == 1:
            assert a[2] == b[2] and a[1] == b[1]
