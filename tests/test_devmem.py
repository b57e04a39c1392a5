"""Host-only: the owners of the engine's device memory and the staging helper (altro-cpp_amd/csrc/altro_devmem.hpp).

tests/cpp/devmem_driver.cpp includes the header and defines the HIP entry points it calls as host stubs -- malloc / free with
a book of live blocks, memcpy, an allocation and a copy that can be told to fail at their k-th call -- so no GPU and no HIP
runtime is involved.  It is built twice with plain g++ against the HIP API header, once with -Wall -Werror and once more with
-fsanitize=address,undefined, and run directly both times; every expectation holds for both programs, and the sanitizer build
must have nothing to report.  A staged block is exactly total() doubles, so a wrong offset is an out-of-bounds access there; a
host array is exactly its elements (ints, bytes and statistics structs included), so a copy that is a byte too long is one too.
Shapes: n = 3, m = 2, B = 5, steps = 2, cycles = 3, shift = 2 (tests/test_part_offsets.py has the offsets written out).
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "altro-cpp_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
ARGS = [str(v) for v in (3, 2, 5, 2, 3, 2)]  # n m B steps cycles shift
# name -> doubles of the block: every named layout whole, and with some of its parts absent
LAYOUTS = dict(track_stage=139, track_stage_sparse=55, tracked_run=354, tracked_run_sparse=354, plain_run=233, plain_run_sparse=165,
               cov_stage=350, cov_stage_sparse=69, inflate_stage=45, inflate_stage_shared=21, ms_best_stage=100, ms_best_stage_sparse=20,
               perturb_stage=20, advance_stage=30, advance_stage_sparse=15, advance_stage_empty=0, reference_stage=75,
               reference_stage_sparse=45,
               # the layouts with ints, bytes and statistics structs in them (DoublesFor: int[5] takes 3 doubles, unsigned char[5]
               # takes 1, int[15] takes 8; TrackStats is 5 doubles, EnsembleStats 7); every host array exactly as long as its elements
               # tracked: 5 5 | age: 3 | bounds: 2 2 | mask: 1 | reason: 3 | lookahead statistics: 5 5
               trigger_stage=61,
               trigger_stage_sparse=25,  # a device caller's: only the lookahead's statistics
               # Sigma0: 5 9 | W: 5 2 9 | bounds: 4 | mean: 5 3 3 | mom2: 5 3 9 | alive: 8 | viol_count: 8 | summary: 5 7 | stats: 5 2 5
               ensemble_stage=420,
               noise_stage=225,          # Sigma0: 45 | W: 90 | dx0: 5 2 3 | w: 5 2 2 3
               gauss_stage=2,            # sigma: m
               lqr_stage=198,            # K: 5 2 2 3 | P: 5 3 9 | fail: 3
               lqr_stage_sparse=63,      # K | no P | fail
               mask_stage=1)             # 5 bytes


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def report(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("devmem_" + request.param) / "devmem_driver"
    flags = ["-O1"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-D__HIP_PLATFORM_AMD__", "-I" + ROCM_INCLUDE, "-I" + CSRC,
                        "-o", str(exe), os.path.join(ROOT, "tests", "cpp", "devmem_driver.cpp")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)] + ARGS, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]  # (a sanitizer report goes to stderr and ends the program)
    return json.loads(r.stdout)


def test_moves_and_replacement_free_each_block_once(report):
    o = report["owners"]
    assert o["moved_from_empty"] and o["pinned_ok"]
    # a: 1 live; c's own block beside it; alloc on the live c frees the one it took over
    assert (o["live_after_move"], o["live_after_assign"], o["live_after_realloc"]) == (1, 2, 2)
    assert o["mallocs"] == 5 and o["frees"] == 5 and o["bad_frees"] == 0 and o["live"] == 0


def test_dropping_an_upload_frees_all_of_it(report):
    u = report["upload"]
    assert u["filled"] and u["live_full"] == 7  # 4 in the pool, the path, a track and its spare
    assert u["live_after_drop"] == 0 and u["pointers_null"]


def test_an_upload_that_fails_at_its_kth_allocation_leaves_nothing(report):
    u = report["upload"]
    assert u["every_k_failed"] and u["live_after_failed"] == [0] * 8 and u["bad_frees"] == 0


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_staging_round_trip(report, name):
    r = report[name]
    assert r["total"] == LAYOUTS[name]
    assert r["arrived"], "an input is not at its part's offset"
    assert r["back"], "an output did not come back whole"
    assert r["absent_null"], "an absent part must yield a null pointer"
    # (the block of a tracked run is the one layout whose parts are all fixed: the bounds keep their 2 m doubles)
    assert r["absent_no_room"] or name == "tracked_run_sparse"
    assert r["h2d"] == r["want_h2d"] and r["d2h"] == r["want_d2h"]
    assert r["syncs"] == 1 and r["error"] == 0 and r["live"] == 0


def test_a_part_too_small_for_the_count_is_treated_as_absent(report):
    """A programming error, handled like a part without room: null pointers, nothing copied, no error; an exact fit goes through."""
    s = report["short_part"]
    assert s["nulls"] and s["fits"] and s["untouched"]
    assert s["h2d"] == 2 and s["d2h"] == 0 and s["error"] == 0  # (the two copies are the ones that fit)


def test_a_failed_upload_copy_still_synchronises(report):
    f = report["failed_copy"]
    assert not f["ok_after"]
    assert f["syncs"] == 1 and f["h2d"] == 0 and f["d2h"] == 0  # nothing else is enqueued behind the failure
    assert f["error"] == f["copy_error"] != f["sync_error"]     # the first error, not the wait's
    assert f["syncs_dropped"] == 1                               # no finish(), uploads on the stream: waited for
    assert f["syncs_idle"] == 0 and f["copies_direct"] == 0 and f["direct_same"]
    assert f["live"] == 0 and f["unexpected"] == 0
