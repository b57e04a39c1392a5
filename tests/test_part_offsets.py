"""Host-only: the parts of the device blocks the closed-loop code carves (Parts, TrackedRunParts, TrackStageParts in
altro-cpp_amd/csrc/altro_common.hpp).

Engine::LoopBegin takes the pointers of a tracked run's eight arrays, and Engine::MpcTrack those of the six arrays it stages
for a host caller, from ONE helper that turns element counts into offsets.  tests/cpp/part_offsets_driver.cpp is built against
the header with plain g++ (it must not need HIP) and prints counts and offsets for n = 3, m = 2, B = 5, cycles = 3, shift = 2;
the expectations below are the sums written out by hand.  The other blocks with a named layout -- the other closed-loop runs,
and what CovPropagate, CovInflate, MsGetBest, MsPerturb, Advance and SetReference stage -- follow, for the same numbers
(tests/test_devmem.py sends arrays through every one of them).
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
n, m, B, CYCLES, SHIFT = 3, 2, 5, 3, 2
SD = 5  # doubles of one TrackStats: two ints in one double, then cost, violation, max_dx, max_du


@pytest.fixture(scope="module")
def parts(tmp_path_factory):
    exe = tmp_path_factory.mktemp("part_offsets") / "part_offsets_driver"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I" + CSRC, "-o", str(exe),
                        os.path.join(ROOT, "tests", "cpp", "part_offsets_driver.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)] + [str(v) for v in (n, m, B, CYCLES, SHIFT)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_track_stats_are_five_doubles(parts):
    assert parts["stats_doubles"] == SD


def test_tracked_run_block(parts):
    """X log | U log | one cycle's X | its U | its last state | its disturbance | u_lo, u_hi | statistics [cycles][B]"""
    p = parts["tracked_run"]
    #                X log: 5 (3 2 + 1) 3 | U log: 5 (3 2) 2 | Xc: 5 (2 + 1) 3 | Uc: 5 2 2 | xend: 5 3 | w: 5 2 3 | 2 m | 3 5 5
    assert p["cnt"] == [105, 60, 45, 20, 15, 30, 4, 75]
    assert p["off"] == [0, 105, 165, 210, 230, 245, 275, 279, 354]
    assert p["total"] == 354


def test_track_stage_block(parts):
    """dx0 | w | u_lo, u_hi | X_cl | U_cl | stats for L = B lanes and `shift` steps"""
    p = parts["track_stage"]
    #                dx0: 5 3 | w: 5 2 3 | 2 m | X_cl: 5 (2 + 1) 3 | U_cl: 5 2 2 | stats: 5 5
    assert p["cnt"] == [15, 30, 4, 45, 20, 25]
    assert p["off"] == [0, 15, 45, 49, 94, 114, 139]
    assert p["total"] == 139


def test_an_absent_array_takes_no_room(parts):
    p = parts["track_stage_sparse"]
    assert p["cnt"] == [0, 30, 0, 0, 0, 25]
    assert p["off"] == [0, 0, 30, 30, 30, 30, 55]
    assert p["total"] == 55


def _is(p, cnt):
    """counts as given; every offset is the sum of the counts before it"""
    assert p["cnt"] == cnt
    assert p["off"] == [sum(cnt[:i]) for i in range(len(cnt) + 1)]
    assert p["total"] == sum(cnt)


def test_plain_run_block(parts):
    """X log | U log | w [cycles][B][n] | dU | clearances"""
    #                      X log: 5 (3 2 + 1) 3 | U log: 5 (3 2) 2 | w: 3 5 3 | dU: 2 2 2 | none
    _is(parts["plain_run"], [105, 60, 45, 8, 0])
    assert parts["plain_run"]["off"] == [0, 105, 165, 210, 218, 218]
    _is(parts["plain_run_sparse"], [105, 60, 0, 0, 0])


def test_cov_stage_block(parts):
    """Sigma0 | W | Sigma | sx | su | rpos with 2 steps"""
    #                      Sigma0: 5 9 | W: 5 2 9 | Sigma: 5 3 9 | sx: 5 3 3 | su: 5 2 2 | rpos: 5 3
    _is(parts["cov_stage"], [45, 90, 135, 45, 20, 15])
    assert parts["cov_stage"]["off"] == [0, 45, 135, 270, 315, 335, 350]
    #                      no Sigma0 | one shared W: 9 | no Sigma | sx | no su | rpos
    _is(parts["cov_stage_sparse"], [0, 9, 0, 45, 0, 15])
    assert parts["cov_stage_sparse"]["off"] == [0, 0, 9, 9, 54, 54, 69]


def test_two_part_blocks(parts):
    _is(parts["inflate_stage"], [30, 15])          # base: 5 2 3 | rpos: 5 (2 + 1)
    _is(parts["inflate_stage_shared"], [6, 15])    # base: 1 2 3
    _is(parts["advance_stage"], [15, 15])          # x0: 5 3 | w: 5 3
    _is(parts["advance_stage_sparse"], [0, 15])
    _is(parts["reference_stage"], [45, 30])        # Xref: 15 points of 3 | Uref: 15 points of 2
    _is(parts["reference_stage_sparse"], [45, 0])
    _is(parts["perturb_stage"], [20])              # dU: 5 2 2


def test_get_best_stage_block(parts):
    """X [P][N + 1][n] | U [P][N][m] | statistics, P = 5 problems, N = 2"""
    _is(parts["ms_best_stage"], [45, 20, 35])      # 5 3 3 | 5 2 2 | 5 7
    assert parts["ms_best_stage"]["off"] == [0, 45, 65, 100]
    _is(parts["ms_best_stage_sparse"], [0, 20, 0])


def test_run_int_block(parts):
    """iterations | statuses | winners | reason log | ages | reasons | next mask, in ints (B = 5, 3 cycles)"""
    _is(parts["run_ints"], [15, 15, 0, 0, 0, 0, 0])                 # plain and tracked runs: two logs of 5 3
    _is(parts["run_ints_team"], [15, 15, 0, 0, 0, 0, 0])
    _is(parts["run_ints_multistart"], [15, 15, 3, 0, 0, 0, 0])      # winners: 1 problem (5 starts) x 3 cycles
    #                                   reason log: 3 5 | ages: 5 | reasons: 5 | mask: 5 bytes in 2 ints
    _is(parts["run_ints_triggered"], [15, 15, 0, 15, 5, 5, 2])
    assert parts["run_ints_triggered"]["off"] == [0, 15, 30, 30, 45, 50, 55, 57]


def test_int_and_byte_parts_are_rounded_up_to_doubles(parts):
    """tracked | age | u_lo, u_hi | mask | reason | lookahead statistics;  K | P | fail;  the solve mask"""
    #                             5 5 | ceil(5 / 2) | 2 2 | ceil(5 / 8) | ceil(5 / 2) | 5 5
    _is(parts["trigger_stage"], [25, 3, 4, 1, 3, 25])
    assert parts["trigger_stage"]["off"] == [0, 25, 28, 32, 33, 36, 61]
    _is(parts["trigger_stage_sparse"], [0, 0, 0, 0, 0, 25])
    _is(parts["lqr_stage"], [60, 135, 3])                            # K: 5 2 2 3 | P: 5 (2 + 1) 9 | fail: ceil(5 / 2)
    _is(parts["lqr_stage_sparse"], [60, 0, 3])
    _is(parts["mask_stage"], [1])                                    # ceil(5 / 8)
