"""Host-only: the parts of the device blocks the closed-loop code carves (Parts, TrackedRunParts, TrackStageParts in
altro-cpp_amd/csrc/altro_common.hpp).

Engine::LoopBegin takes the pointers of a tracked run's eight arrays, and Engine::MpcTrack those of the six arrays it stages
for a host caller, from ONE helper that turns element counts into offsets.  tests/cpp/part_offsets_driver.cpp is built against
the header with plain g++ (it must not need HIP) and prints counts and offsets for n = 3, m = 2, B = 5, cycles = 3, shift = 2;
the expectations below are the sums written out by hand.
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
