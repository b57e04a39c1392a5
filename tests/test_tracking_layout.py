"""Host-only: what the problem compiler (altro-cpp_amd/csrc/altro_problem.hpp) makes of tracking costs
(altro_set_lqr_tracking_cost, include/altro_tracking.h).  tests/cpp/tracking_layout_driver.cpp is built with plain g++ and
prints the layouts, n = 3, m = 2, N = 24:
  * a tracking range is ONE cost group whatever the number of knots: Q, R in the shared pool, and q, r, c marked "per knot"
    (2) at elements 0, n, n + m of the knot's reference-term record -- no parameter of theirs in either pool;
  * the same problem written as one ordinary cost per knot still exceeds the cost groups, with the text it always had;
  * the description the kernels receive does not grow."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
N, n, m = 24, 3, 2
OK, UNSUPPORTED = 0, 4
FAST_GENERIC, FAST_NONE, FAST_B = 0, 1, 2
PER_KNOT = 2


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("tracking_layout") / "tracking_layout_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "tracking_layout_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_25_references_are_two_groups(layouts):
    p = layouts["tracking_25"]
    assert p["status"] == OK, p["err"]
    assert (p["ngroups"], p["nclass"], p["nruns"]) == (2, 2, 2)
    assert p["knot_group"] == [0] * N + [1]
    for g, q00 in zip(p["groups"], (1.0, 100.0)):
        assert (g["q_pi"], g["r_pi"], g["c_pi"]) == (PER_KNOT, PER_KNOT, PER_KNOT)
        assert (g["q_off"], g["r_off"], g["c_off"]) == (0, n, n + m)
        assert (g["q_diag"], g["r_diag"], g["Q00"]) == (1, 1, q00)
    # Q and R of the two groups and the four bounds: nothing of q, r, c in the pools
    assert p["npool"] == 2 * (n * n + m * m) + 4 and p["nslots"] == 0
    assert [g["Q_off"] for g in p["groups"]] == [0, n * n + m * m]
    # the stage knots keep the specialised layout of a full control bound; the terms are re-read per knot there
    assert p["fast"] == [FAST_B, FAST_NONE]


def test_ordinary_per_knot_costs_still_exceed_the_groups(layouts):
    p = layouts["ordinary_25"]
    assert (p["status"], p["err"]) == (UNSUPPORTED, "too many distinct cost functions")


def test_last_cost_wins_whichever_kind(layouts):
    p = layouts["mixed"]
    assert p["status"] == OK, p["err"]
    assert p["ngroups"] == 2  # the covered ordinary cost is not counted
    assert p["knot_group"] == [0] * 4 + [1] * (N + 1 - 4)
    ordinary, tracking = p["groups"]
    assert (ordinary["q_pi"], ordinary["r_pi"], ordinary["c_pi"], ordinary["Q00"]) == (0, 0, 0, 3.0)
    assert (tracking["q_pi"], tracking["r_pi"], tracking["c_pi"], tracking["Q00"]) == (PER_KNOT, PER_KNOT, PER_KNOT, 1.0)


def test_the_description_does_not_grow(layouts):
    """CostGroupDesc: 13 ints; ProblemDesc: 12 words, 16 runs of 8, 8 classes of 4 + 4 x 8, 8 groups -- the sizes before
    tracking costs existed (ProblemDesc travels as a kernel argument).  Records are 16-byte multiples."""
    s = layouts["sizes"]
    assert s["CostGroupDesc"] == 13 * 4
    assert s["ProblemDesc"] == 12 * 4 + 16 * 8 * 4 + 8 * (4 + 4 * 8) * 4 + 8 * 13 * 4
    assert s["per_knot"] == PER_KNOT and s["record"] == 6 and s["point"] == 6
