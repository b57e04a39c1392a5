"""Host-only: what the problem compiler (altro-cpp_amd/csrc/altro_problem.hpp) makes of knot constraints
(altro_add_knot_constraint, include/altro_knot_params.h).  tests/cpp/knot_params_layout_driver.cpp is built with plain g++
and prints the layouts, n = 3, m = 2, N = 24:
  * problems.moving_obstacles is 3 classes and 3 runs whatever the number of knots; both constraints carry the per-knot
    marker (3) with param_off 0 and 6 in the knot's record, and no parameter of theirs sits in either pool;
  * the stage runs keep the specialised layouts of a full control bound and of circle + full bound;
  * the same problem written as one ordinary constraint per knot still exceeds the knot classes, with the text it always had;
  * the description the kernels receive does not grow."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
N, n, m = 24, 3, 2
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 4
FAST_NONE, FAST_B, FAST_CB, FAST_GENERIC = 1, 2, 3, 0
GOAL, BOUND, CIRCLE = 1, 2, 3
PER_KNOT = 3


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("knot_params_layout") / "knot_params_layout_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "knot_params_layout_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_constants_match_the_c_header(A):
    assert (A.CON_GOAL, A.CON_CONTROL_BOUND, A.CON_CIRCLE) == (GOAL, BOUND, CIRCLE)
    assert (A.INVALID_ARG, A.UNSUPPORTED) == (INVALID_ARG, UNSUPPORTED)


def test_moving_obstacles_is_three_classes_and_three_runs(layouts):
    p = layouts["moving_obstacles"]
    assert p["status"] == OK, p["err"]
    assert (p["nclass"], p["nruns"]) == (3, 3)
    assert p["knot_class"] == [0] + [1] * (N - 1) + [2]
    assert [(r["k_begin"], r["k_end"], r["cls"]) for r in p["runs"]] == [(0, 1, 0), (1, N, 1), (N, N + 1, 2)]
    # knot 0: the bound; knots 1 .. N-1: circle then bound (registration order); knot N: none
    first, stage, last = p["classes"]
    assert [c["kind"] for c in first["cons"]] == [BOUND] and first["nrows"] == 4
    assert [c["kind"] for c in stage["cons"]] == [CIRCLE, BOUND] and stage["nrows"] == 6
    assert last["cons"] == [] and last["nrows"] == 0
    circle, bound = stage["cons"]
    assert (circle["per_instance"], circle["param_off"], circle["p"], circle["row_off"]) == (PER_KNOT, 0, 2, 0)
    assert (bound["per_instance"], bound["param_off"], bound["p"], bound["row_off"]) == (PER_KNOT, 6, 4, 2)
    assert first["cons"][0]["param_off"] == 6 and first["cons"][0]["per_instance"] == PER_KNOT
    # every bound of a knot bound is "finite": all 2m rows, so the specialised layouts still name the runs
    assert (bound["lo_mask"], bound["hi_mask"]) == (3, 3)
    assert [r["fast"] for r in p["runs"]] == [FAST_B, FAST_CB, FAST_NONE]
    # Q, R of the two tracking groups and nothing else in the shared pool; no per-instance slot
    assert p["npool"] == 2 * (n * n + m * m) and p["nslots"] == 0
    assert p["con_knot_off"] == [0, 6] and p["knot_record"] == 10 and p["con_p"] == [2, 4]
    assert p["total_rows"] == 4 + 6 * (N - 1)


def test_ordinary_per_knot_constraints_still_exceed_the_classes(layouts):
    p = layouts["ordinary_per_knot"]
    assert (p["status"], p["err"]) == (UNSUPPORTED, "too many distinct knot-point classes")


def test_knot_and_ordinary_constraints_side_by_side(layouts):
    p = layouts["mixed"]
    assert p["status"] == OK, p["err"]
    assert (p["nclass"], p["nruns"]) == (3, 3)
    assert p["con_knot_off"] == [0, -1, 4] and p["knot_record"] == 8  # 4 + 3, rounded up to a pair
    first, stage, last = p["classes"]
    b, c = stage["cons"]
    assert (b["kind"], b["per_instance"], b["param_off"]) == (BOUND, PER_KNOT, 0)
    assert (c["kind"], c["per_instance"], c["param_off"]) == (CIRCLE, 0, 2 * (n * n + m * m))  # the ordinary circle: the pool
    g, = last["cons"]
    assert (g["kind"], g["per_instance"], g["param_off"], g["p"]) == (GOAL, PER_KNOT, 4, n)
    assert p["npool"] == 2 * (n * n + m * m) + 3 and p["nslots"] == 0


def test_nparams_must_fit_the_kind(layouts):
    p = layouts["bad_nparams"]
    assert p["status"] == INVALID_ARG and "control bound" in p["err"]


def test_the_description_does_not_grow(layouts):
    """ConDesc: 8 words; KnotClass: 4 words + 4 ConDesc; ProblemDesc: 12 words, 16 runs of 8, 8 classes, 8 groups of 13 -- the
    sizes of the commit before knot constraints existed, printed from a build of it (ProblemDesc travels to the kernels)."""
    s = layouts["sizes"]
    assert (s["ConDesc"], s["KnotClass"], s["ProblemDesc"]) == (32, 144, 2128)
    assert s["marker"] == PER_KNOT
