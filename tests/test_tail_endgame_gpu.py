"""The endgame of the persistent tail (TwinCtl, altro_kernels.hpp): the minimum share of a split is a policy value
(ALTRO_TWIN_MIN at build time, ALTRO_HIP_TWIN_MIN per process, clamped to kTwinMinFloor), and a pool workgroup shows its
segment as soon as its clone is in memory, so splits cascade in clone time instead of iteration time.

Nothing of that may change a result: every iteration is still executed exactly once, on the inputs the sequential order
gives it.  Each case is compared with a launch without twins (ALTRO_HIP_TWIN=0) bit for bit: trajectories, gains,
multipliers, penalties, stored constraint values, expansion records, knot costs, every statistic.  Every run is two solves
through one handle (mailboxes and shadow columns are reused) in a fresh child process (the switches are read once per
process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 3   # kTwinMinFloor (tests/test_tail_endgame_policy.py asks the library for it)

_SCRIPT = r'''
import importlib, sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
A = g.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
make = lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)
case, path = sys.argv[1], sys.argv[2]
cases = {"turn90_16": lambda: P.batch_turn90(make, batch=16, seed=P.SEED_BASE + 3),        # one straggler (instance 9), a pool far larger than the batch
         "turn90_64": lambda: P.batch_turn90(make, batch=64, seed=P.SEED_BASE + 3),        # stragglers 9, 18, 41, 48 compete for the pool
         "obstacles_48": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F64),   # lock-step speculation (circle constraints)
         "obstacles_48_r32": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F32)}   # fp32 records
s = cases[case]()
for rep in range(2):   # (the second solve reuses mailboxes and shadow columns)
    s.reset_trajectory()
    s.solve()
out = {}
X, U = s.get_trajectory()
st = s.get_stats()
tm = s.get_timing()
out["X"] = X; out["U"] = U
K, d = s.get_gains()
out["K"] = K; out["d"] = d
out["lam"] = s.get_duals(); out["pen"] = s.get_penalties(); out["c"] = s.get_constraint_values()
for f in st.dtype.names:
    out["st_" + f] = st[f]
for k in (0, 50, 100):
    e = s.get_expansion(k)
    for key, v in e.items():
        if k < 100 or key in ("lxx", "lx"):   # (the terminal knot has no dynamics and no control blocks)
            out["exp%%d_%%s" %% (k, key)] = v
out["costs"] = s.get_knot_costs()
out["tw_"] = np.array([tm["twin_workgroups"], tm["twin_claims"], tm["twin_handovers"]])
out["ms_"] = np.array([tm["total_ms"]])
s.close()
np.savez(path, **out)
'''

CASES = ["turn90_16", "turn90_64", "obstacles_48", "obstacles_48_r32"]
_SWITCHES = ("ALTRO_HIP_TWIN", "ALTRO_HIP_TWIN_MIN", "ALTRO_HIP_TWIN_DEPTH", "ALTRO_HIP_TWIN_MISCLAIM", "ALTRO_HIP_DEBUG_POISON")
_solo = {}


def _run(tmp_path, case, tag, env_extra):
    out = str(tmp_path / f"{case}_{tag}.npz")
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}   # (a run has the switches its test names, no others)
    subprocess.run([sys.executable, "-c", _SCRIPT % ROOT, case, out], check=True, env=dict(env, **env_extra), timeout=600)
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def _reference(tmp_path, case):
    """the run without twins: computed once per case, shared by the tests"""
    if case not in _solo:
        _solo[case] = _run(tmp_path, case, "solo", {"ALTRO_HIP_TWIN": "0"})
        assert _solo[case]["tw_"][0] == 0
    return _solo[case]


def _same(got, ref, what):
    assert sorted(got) == sorted(ref)
    for k in ref:
        if k.endswith("_"):   # (pool size, claims, joints, milliseconds)
            continue
        assert np.array_equal(got[k], ref[k]), (what, k, np.abs(np.asarray(got[k], float) - np.asarray(ref[k], float)).max())


def _report(case, tag, got, ref):
    print(f"{case} [{tag}]: pool / claims / confirmed joints {got['tw_'].tolist()}, ms with / without splitting "
          f"{got['ms_'][0]:.3f} / {ref['ms_'][0]:.3f}")


@pytest.mark.parametrize("case", CASES)
def test_default_minimum_is_bit_identical(tmp_path, case):
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, "default", {})
    _report(case, "default", got, ref)
    _same(got, ref, "default")
    # no streak of these batches breaks before the iteration cap: every claim is confirmed at its joint
    assert got["tw_"][0] > 0 and got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]


def test_cascade_to_the_floor(tmp_path):
    """one straggler, 64 pool workgroups, the smallest share and the deepest line of claims: the cascade runs as far as the
    policy lets it, every claim is confirmed, and there are more of them than with shares of 12 iterations"""
    case = "turn90_16"
    ref = _reference(tmp_path, case)
    fine = _run(tmp_path, case, "floor_depth5", {"ALTRO_HIP_TWIN_MIN": str(FLOOR), "ALTRO_HIP_TWIN_DEPTH": "5"})
    coarse = _run(tmp_path, case, "min12_depth5", {"ALTRO_HIP_TWIN_MIN": "12", "ALTRO_HIP_TWIN_DEPTH": "5"})
    _report(case, f"min {FLOOR} depth 5", fine, ref)
    _report(case, "min 12 depth 5", coarse, ref)
    _same(fine, ref, "floor, depth 5")
    _same(coarse, ref, "min 12, depth 5")
    assert fine["tw_"][2] == fine["tw_"][1] and coarse["tw_"][2] == coarse["tw_"][1], (fine["tw_"], coarse["tw_"])
    assert fine["tw_"][1] > coarse["tw_"][1], (fine["tw_"], coarse["tw_"])


@pytest.mark.parametrize("case", ["turn90_64", "obstacles_48", "obstacles_48_r32"])
def test_floor_is_bit_identical(tmp_path, case):
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, "floor", {"ALTRO_HIP_TWIN_MIN": str(FLOOR)})
    _report(case, f"min {FLOOR}", got, ref)
    _same(got, ref, "floor")
    assert got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64", "obstacles_48_r32"])
def test_floor_with_poisoned_memory(tmp_path, case):
    """shadow columns, LDS and the candidate buffer full of NaN words before every solve: a clone of a clone of a clone,
    taken the moment its source was written, computes with nothing the solve has not written"""
    ref = _reference(tmp_path, case)
    env = {"ALTRO_HIP_DEBUG_POISON": "7ff80000,mix", "ALTRO_HIP_TWIN_MIN": str(FLOOR)}
    if case == "turn90_16":
        env["ALTRO_HIP_TWIN_DEPTH"] = "5"
    got = _run(tmp_path, case, "poisoned", env)
    _report(case, "poisoned", got, ref)
    _same(got, ref, "poisoned")
    assert got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64"])
@pytest.mark.parametrize("k", [1, 2])
def test_refused_claimers_take_their_line_down(tmp_path, case, k):
    """ALTRO_HIP_TWIN_MISCLAIM=k lets every k-th claim assume a regularisation one ulp off.  Its claimer has shown its
    segment before anybody checked that assumption, and others have claimed from it: the joint must refuse it, everything
    down its line must drop its column, and the result is still the sequential one."""
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, f"misclaim{k}", {"ALTRO_HIP_TWIN_MISCLAIM": str(k), "ALTRO_HIP_TWIN_MIN": str(FLOOR)})
    _report(case, f"misclaim {k}", got, ref)
    _same(got, ref, f"misclaim {k}")
    assert got["tw_"][1] > 0 and got["tw_"][2] < got["tw_"][1], got["tw_"]


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64"])
def test_former_policy_is_still_there(tmp_path, case):
    """shares of 12 iterations, one twin per primary"""
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, "min12_depth1", {"ALTRO_HIP_TWIN_MIN": "12", "ALTRO_HIP_TWIN_DEPTH": "1"})
    _report(case, "min 12 depth 1", got, ref)
    _same(got, ref, "min 12, depth 1")
    assert got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]
