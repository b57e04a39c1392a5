"""The trigger rule of include/altro_trigger.h on the host: altro_common.hpp's trigger_reason (THE function k_mpc_trigger calls
too) through tests/cpp/trigger_rule_driver.cpp, built with plain g++, against the numpy statement of tests/_trigger_common.py.
This is where NaN, the infinities and values one ulp around a tolerance are covered.  Needs no GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _trigger_common as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
STATS = np.dtype([("status", np.int32), ("violation", np.float64), ("max_dx", np.float64)])
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("trigger_rule") / "trigger_rule_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "trigger_rule_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(rows, path):
        np.ascontiguousarray(rows, dtype=np.float64).tofile(str(path))
        r = subprocess.run([str(exe), str(path), str(len(rows))], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        return [int(v) for v in lines[0].split()], np.array([int(v) for v in lines[1:]], dtype=np.int32)
    return run


def _row(rule, age=0, tracked=None, status=TG.SOLVED, ahead=None):
    """(the driver's 15 doubles, the numpy rule's answer for this one instance)"""
    t = np.zeros(1, dtype=STATS)
    a = np.zeros(1, dtype=STATS)
    if tracked is not None:
        t[0] = tracked
    if ahead is not None:
        a[0] = (ahead[0], ahead[1], 0.0)
    want = TG.reason(rule, 1, None if tracked is None else t, [age], [status], None if ahead is None else a)[0]
    assert want == TG.reason_loop(rule, 1, None if tracked is None else t, [age], [status], None if ahead is None else a)[0]
    return [rule["max_age"], rule["dx_tol"], rule["viol_tol"], rule["on_unsolved"], rule["lookahead"], rule["ahead_tol"], age,
            0.0 if tracked is None else 1.0, t["status"][0], t["violation"][0], t["max_dx"][0], status,
            0.0 if ahead is None else 1.0, a["status"][0], a["violation"][0]], int(want)


QUIET = (TG.UNSOLVED_STATUS, 0.0, 0.0)  # a tracked segment that triggers nothing: (status, violation, max_dx)


def _cases():
    """name -> (row arguments, the reason the issue's text gives)"""
    R = TG.rule_dict
    up = lambda v: float(np.nextafter(v, INF))  # noqa: E731
    full = R(max_age=3, dx_tol=1e-3, viol_tol=1e-4, on_unsolved=1, lookahead=4, ahead_tol=1e-4)
    cases = {
        "nothing": (dict(rule=full, age=0, tracked=QUIET, ahead=(1, 0.0)), 0),
        # each criterion alone
        "age": (dict(rule=full, age=3, tracked=QUIET, ahead=(1, 0.0)), TG.AGE),
        "deviation": (dict(rule=full, tracked=(1, 0.0, 2e-3), ahead=(1, 0.0)), TG.DEVIATION),
        "violation": (dict(rule=full, tracked=(1, 2e-4, 0.0), ahead=(1, 0.0)), TG.VIOLATION),
        "state_limit": (dict(rule=full, tracked=(2, 0.0, 0.0), ahead=(1, 0.0)), TG.LIMIT),
        "control_limit": (dict(rule=full, tracked=(3, 0.0, 0.0), ahead=(1, 0.0)), TG.LIMIT),
        "unsolved": (dict(rule=full, tracked=QUIET, status=5, ahead=(1, 0.0)), TG.UNSOLVED),
        "unsolved_off": (dict(rule=R(max_age=3), tracked=QUIET, status=5), 0),
        "ahead_violation": (dict(rule=full, tracked=QUIET, ahead=(1, 2e-4)), TG.AHEAD),
        "ahead_limit": (dict(rule=full, tracked=QUIET, ahead=(2, 0.0)), TG.AHEAD),
        "ahead_nan": (dict(rule=full, tracked=QUIET, ahead=(1, NAN)), TG.AHEAD),
        "ahead_off": (dict(rule=R(max_age=3, ahead_tol=1e-4), tracked=QUIET, ahead=(2, 1.0)), 0),
        # all together
        "all": (dict(rule=full, age=7, tracked=(2, 1.0, 1.0), status=1, ahead=(3, 1.0)),
                TG.AGE | TG.DEVIATION | TG.VIOLATION | TG.LIMIT | TG.UNSOLVED | TG.AHEAD),
        # exactly at a tolerance, and one ulp above
        "dx_at_tol": (dict(rule=full, tracked=(1, 0.0, 1e-3)), 0),
        "dx_ulp_above": (dict(rule=full, tracked=(1, 0.0, up(1e-3))), TG.DEVIATION),
        "viol_at_tol": (dict(rule=full, tracked=(1, 1e-4, 0.0)), 0),
        "viol_ulp_above": (dict(rule=full, tracked=(1, up(1e-4), 0.0)), TG.VIOLATION),
        "ahead_at_tol": (dict(rule=full, tracked=QUIET, ahead=(1, 1e-4)), 0),
        "ahead_ulp_above": (dict(rule=full, tracked=QUIET, ahead=(1, up(1e-4))), TG.AHEAD),
        "zero_tol_zero_dx": (dict(rule=R(max_age=3, dx_tol=0.0, viol_tol=0.0), tracked=QUIET), 0),
        "zero_tol_tiny_dx": (dict(rule=R(max_age=3, dx_tol=0.0, viol_tol=0.0), tracked=(1, 0.0, 5e-324)), TG.DEVIATION),
        # NaN and +inf
        "dx_nan": (dict(rule=full, tracked=(1, 0.0, NAN)), TG.DEVIATION),
        "dx_inf": (dict(rule=full, tracked=(1, 0.0, INF)), TG.DEVIATION),
        "viol_nan": (dict(rule=full, tracked=(1, NAN, 0.0)), TG.VIOLATION),
        "viol_inf": (dict(rule=full, tracked=(1, INF, 0.0)), TG.VIOLATION),
        "inf_tol_inf_dx": (dict(rule=R(max_age=3, dx_tol=INF), tracked=(1, 0.0, INF)), 0),
        "inf_tol_nan_dx": (dict(rule=R(max_age=3, dx_tol=INF), tracked=(1, 0.0, NAN)), TG.DEVIATION),
        # negative tolerances: off, whatever the value
        "dx_off": (dict(rule=R(max_age=3, dx_tol=-1.0, viol_tol=1e-4), tracked=(1, 0.0, NAN)), 0),
        "viol_off": (dict(rule=R(max_age=3, dx_tol=1e-3, viol_tol=-1e-300), tracked=(1, INF, 0.0)), 0),
        "off_but_limit": (dict(rule=R(max_age=3), tracked=(2, NAN, NAN)), TG.LIMIT),
        # the age boundary
        "age_below": (dict(rule=full, age=2, tracked=QUIET), 0),
        "age_at": (dict(rule=full, age=3, tracked=QUIET), TG.AGE),
        "age_one": (dict(rule=R(max_age=1), age=1), TG.AGE),
        "age_zero_of_one": (dict(rule=R(max_age=1), age=0), 0),
        # tracked == NULL: the three tracked criteria are off
        "no_tracked": (dict(rule=full, age=1), 0),
        "no_tracked_age": (dict(rule=full, age=4, status=1), TG.AGE | TG.UNSOLVED),
    }
    return cases


def test_rule_against_numpy(driver, tmp_path):
    cases = _cases()
    rows, numpy_says, issue_says = [], [], []
    for name, (args, want) in cases.items():
        row, got = _row(**args)
        assert got == want, (name, got, want)  # the numpy statement gives what the issue's text gives
        rows.append(row)
        numpy_says.append(got)
        issue_says.append(want)
    bits, got = driver(rows, tmp_path / "rows.bin")
    assert bits == [TG.FIRST, TG.AGE, TG.DEVIATION, TG.VIOLATION, TG.LIMIT, TG.UNSOLVED, TG.AHEAD]
    bad = [(name, int(g), w) for name, g, w in zip(cases, got, numpy_says) if g != w]
    assert not bad, bad
    assert not (got & TG.FIRST).any()  # the rule never sets FIRST: that is the run's own


def test_rule_on_random_rows(driver, tmp_path):
    """4000 random rows with the special values mixed in, the vectorised numpy statement against the driver"""
    rng = np.random.RandomState(11)
    special = np.array([0.0, 1e-3, np.nextafter(1e-3, 1), np.nextafter(1e-3, 0), NAN, INF, -1.0, 1e-4, 5e-324])
    M = 4000
    pick = lambda: special[rng.randint(0, special.size, M)]  # noqa: E731
    rows = np.zeros((M, 15))
    rows[:, 0] = rng.randint(1, 5, M)
    rows[:, 1] = np.where(rng.rand(M) < 0.3, -1.0, 1e-3)
    rows[:, 2] = np.where(rng.rand(M) < 0.3, -0.5, 1e-4)
    rows[:, 3] = rng.randint(0, 2, M)
    rows[:, 4] = rng.randint(0, 3, M)
    rows[:, 5] = 1e-4
    rows[:, 6] = rng.randint(0, 6, M)
    rows[:, 7] = 1.0
    rows[:, 8] = rng.randint(1, 4, M)
    rows[:, 9], rows[:, 10] = pick(), pick()
    rows[:, 11] = rng.randint(0, 3, M)
    rows[:, 12] = 1.0
    rows[:, 13] = rng.randint(1, 3, M)
    rows[:, 14] = pick()
    _, got = driver(rows, tmp_path / "random.bin")
    groups = {}
    for r in range(M):  # the numpy statement takes one rule: group the rows by theirs
        groups.setdefault(tuple(rows[r, :6]), []).append(r)
    for key, idx in groups.items():
        rule = TG.rule_dict(int(key[0]), key[1], key[2], int(key[3]), int(key[4]), key[5])
        t = np.zeros(len(idx), dtype=STATS)
        a = np.zeros(len(idx), dtype=STATS)
        t["status"], t["violation"], t["max_dx"] = rows[idx, 8], rows[idx, 9], rows[idx, 10]
        a["status"], a["violation"] = rows[idx, 13], rows[idx, 14]
        want = TG.reason(rule, len(idx), t, rows[idx, 6], rows[idx, 11], a)
        assert np.array_equal(want, got[idx]), key
        assert np.array_equal(want, TG.reason_loop(rule, len(idx), t, rows[idx, 6], rows[idx, 11], a)), key
    assert len(set(got.tolist())) > 20  # many different reasons occurred


def test_constants_match(A):
    """the header's ALTRO_TRIGGER_* enum, the binding's TRIGGER_* and tests/_trigger_common.py are the same bits"""
    src = open(os.path.join(ROOT, "include", "altro_trigger.h")).read()
    for name in ("FIRST", "AGE", "DEVIATION", "VIOLATION", "LIMIT", "UNSOLVED", "AHEAD"):
        m = re.search(r"\bALTRO_TRIGGER_%s = (\d+)" % name, src)
        assert m, name
        assert int(m.group(1)) == getattr(A, "TRIGGER_" + name) == getattr(TG, name), name
