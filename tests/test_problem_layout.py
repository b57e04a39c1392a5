"""Host-only: the problem compiler (altro-cpp_amd/csrc/altro_problem.hpp) lays a problem out by the reference's rules.

tests/cpp/problem_layout_driver.cpp is built against the header with plain g++ (the header must not need HIP) and prints the
compiled layout of a few small problems; the expectations below are worked out by hand from the reference's rules, for
n = 3, m = 2, N = 8:
  * the last SetCostFunction on a knot wins (altro/problem/problem.hpp:113-127);
  * rows of a knot: equalities first, then inequalities, each in insertion order (al_cost.hpp:267-272);
  * a control bound keeps only its finite entries (examples/basic_constraints.hpp:138-145);
  * an LQR cost group takes n*n + m*m + n + m + 1 = 19 shared parameters: Q, R, q = -Q xref, r = -R uref, c."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
N = 8
LQR_PARAMS = 3 * 3 + 2 * 2 + 3 + 2 + 1
OK, INVALID_ARG, NOT_READY, UNSUPPORTED = 0, 1, 3, 4  # altro_status (include/altro_hip.h)
GOAL, CONTROL_BOUND = 1, 2  # altro_constraint_kind
FAST_GENERIC, FAST_NONE, FAST_B = 0, 1, 2  # FastKind (altro_common.hpp)


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("problem_layout") / "problem_layout_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "problem_layout_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_header_needs_no_hip():
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-x", "c++", "-include",
                        os.path.join(CSRC, "altro_problem.hpp"), os.devnull], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]


def test_unicycle_turn(layouts):
    p = layouts["unicycle_turn"]
    assert p["status"] == OK, p["err"]
    assert (p["ngroups"], p["nclass"], p["nruns"]) == (2, 2, 2)
    assert p["runs"][0] == {"k_begin": 0, "k_end": N, "cls": 0, "rowbase": 0, "fast": FAST_B}
    assert p["runs"][1] == {"k_begin": N, "k_end": N + 1, "cls": 1, "rowbase": 4 * N, "fast": FAST_GENERIC}
    assert p["total_rows"] == 4 * N + 3
    assert p["knot_rowbase"] == [4 * k for k in range(N + 1)]
    assert p["knot_class"] == [0] * N + [1]
    assert [c["nrows"] for c in p["classes"]] == [4, 3]
    assert (p["con_kb"], p["con_ke"], p["con_p"], p["con_eq"]) == ([0, N], [N, N + 1], [4, 3], [0, 1])
    assert p["nslots"] == 0 and p["npool"] == 2 * LQR_PARAMS + 4 + 3


def test_last_set_cost_function_wins(layouts):
    p = layouts["last_cost_wins"]  # Q = diag(7, 8, 9) on [0, 4), then diag(1, 2, 3) on [0, N), diag(100, ..) on the last knot
    assert p["status"] == OK, p["err"]
    assert (p["ngroups"], p["nclass"], p["nruns"]) == (2, 2, 2)  # the covered cost is not counted
    assert p["npool"] == 2 * LQR_PARAMS and 7.0 not in p["pool"]
    assert p["pool"][p["groups"][0]["Q_off"]] == 1.0 and p["pool"][p["groups"][1]["Q_off"]] == 100.0
    assert p["knot_class"] == [0] * N + [1]
    q = layouts["last_cost_wins_partly"]  # diag(7, ..) everywhere, then diag(1, ..) on [2, 5)
    assert q["status"] == OK, q["err"]
    assert (q["ngroups"], q["nclass"], q["nruns"]) == (2, 2, 3)
    assert q["knot_class"] == [0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert [q["classes"][c]["cost_group"] for c in (0, 1)] == [0, 1]
    assert q["pool"][q["groups"][0]["Q_off"]] == 7.0 and q["pool"][q["groups"][1]["Q_off"]] == 1.0


def test_row_order_equalities_first(layouts):
    p = layouts["row_order"]  # a control bound on [2, 6), added first; a goal on knot 4
    assert p["status"] == OK, p["err"]
    assert p["knot_class"] == [0, 0, 1, 1, 2, 1, 0, 0, 0]
    both = p["classes"][2]["cons"]
    assert [(c["kind"], c["type"], c["row_off"], c["p"]) for c in both] == [(GOAL, 0, 0, 3), (CONTROL_BOUND, 1, 3, 4)]
    assert p["classes"][2]["nrows"] == 7
    assert p["knot_rowbase"] == [0, 0, 0, 4, 8, 15, 19, 19, 19] and p["total_rows"] == 19
    # insertion order, whatever the order of the rows
    assert (p["con_kb"], p["con_ke"], p["con_p"], p["con_eq"]) == ([2, 4], [6, 5], [4, 3], [0, 1])


def test_infinite_bounds_are_dropped(layouts):
    p = layouts["infinite_bound"]  # lower (-1.5, -2.5), upper (max(), 2.5)
    assert p["status"] == OK, p["err"]
    c = p["classes"][0]["cons"][0]
    assert (c["lo_mask"], c["hi_mask"]) == (0b11, 0b10)
    assert c["p"] == bin(c["lo_mask"]).count("1") + bin(c["hi_mask"]).count("1") == 3
    assert c["param_off"] == LQR_PARAMS and p["pool"][c["param_off"]:] == [-1.5, -2.5, 2.5]
    assert p["total_rows"] == 3 * N
    assert [r["fast"] for r in p["runs"]] == [FAST_GENERIC, FAST_NONE]  # not kFastB: a bound is missing


def test_off_diagonal_cost_is_generic(layouts):
    p = layouts["off_diagonal"]
    assert p["status"] == OK, p["err"]
    assert (p["groups"][0]["q_diag"], p["groups"][0]["r_diag"]) == (0, 1)
    assert [r["fast"] for r in p["runs"]] == [FAST_GENERIC]  # (kFastNone with a diagonal Q: see the last run above)


def test_per_instance_goal_parameters(layouts):
    p = layouts["per_instance_goal"]  # B = 3, goals (11, 12, 13), (21, 22, 23), (31, 32, 33)
    assert p["status"] == OK, p["err"]
    assert p["nslots"] == 3 and p["slots"] == [[11, 21, 31], [12, 22, 32], [13, 23, 33]]
    c = p["classes"][1]["cons"][0]
    assert (c["kind"], c["per_instance"], c["param_off"]) == (GOAL, 1, 0)
    assert p["npool"] == LQR_PARAMS  # nothing of the goal in the shared pool


@pytest.mark.parametrize("case, status, text", [
    ("no_cost_at_knot_5", NOT_READY, "cost function missing at knot 5 (Problem::IsFullyDefined)"),
    ("too_many_classes", UNSUPPORTED, "too many distinct knot-point classes"),
    ("goal_with_two_parameters", INVALID_ARG, "goal constraint needs n parameters"),
    ("user_cost_without_user_types", INVALID_ARG,
     "this model defines no UserCost (altro_set_user_cost needs a user model whose source defines ALTRO_USER_COST)")])
def test_refusals(layouts, case, status, text):
    assert (layouts[case]["status"], layouts[case]["err"]) == (status, text)
