"""Rejection streaks split more than once inside the persistent tail kernel (TwinCtl, altro_kernels.hpp).

A streak is a chain of segments, one workgroup each; an idle pool workgroup claims the second half of what is left of ANY
published segment, the primary's or another pool workgroup's.  Every iteration is still executed exactly once, on the inputs
the sequential order gives it, so NOTHING may differ from a launch without twins (ALTRO_HIP_TWIN=0): trajectories, gains,
multipliers, penalties, stored constraint values, expansion records, knot costs, every statistic.  Each run is a fresh child
process (the switches are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r'''
import importlib, sys, numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
A = g.load_package()
P = importlib.import_module("altro_cpp_amd.problems")
make = lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d)
case, reps, path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
cases = {"turn90_16": lambda: P.batch_turn90(make, batch=16, seed=P.SEED_BASE + 3),        # one straggler (instance 9), 16+ pool workgroups
         "turn90_64": lambda: P.batch_turn90(make, batch=64, seed=P.SEED_BASE + 3),        # stragglers 9, 18, 41, 48 compete for the pool
         "obstacles_48": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F64),   # lock-step speculation (circle constraints)
         "obstacles_48_r32": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F32),   # fp32 records
         "turn90_2304": lambda: P.batch_turn90(make, batch=2304, seed=P.SEED_BASE + 3)}    # behind the chains of sweeps, CUs scarce
s = cases[case]()
for rep in range(reps):   # (a second solve reuses mailboxes and shadow columns)
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

_REPS = {"turn90_16": 2, "turn90_64": 2}
_solo = {}


def _run(tmp_path, case, tag, env_extra):
    out = str(tmp_path / f"{case}_{tag}.npz")
    subprocess.run([sys.executable, "-c", _SCRIPT % ROOT, case, str(_REPS.get(case, 1)), out], check=True,
                   env=dict(os.environ, **env_extra), timeout=600)
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


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64", "obstacles_48", "obstacles_48_r32"])
def test_split_streaks_are_bit_identical(tmp_path, case):
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, "split", {})
    _report(case, "default", got, ref)
    assert got["tw_"][0] > 0
    _same(got, ref, "default")
    if case == "turn90_16":
        # one straggler and a pool far larger than the batch: both halves of its streak were split again
        assert got["tw_"][0] >= 16 and got["tw_"][1] >= 3, got["tw_"]
    if case == "turn90_64":
        # four stragglers (instances 9, 18, 41, 48): more claims than one twin each
        assert got["tw_"][1] > 4, got["tw_"]
    # no streak of these batches breaks before the iteration cap: every claim is confirmed at its joint
    assert got["tw_"][2] == got["tw_"][1], got["tw_"]


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64", "obstacles_48_r32"])
def test_split_streaks_with_poisoned_memory(tmp_path, case):
    """shadow columns, LDS and the candidate buffer full of NaN words before every solve: a clone of a clone computes with
    nothing the solve has not written"""
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, "poisoned", {"ALTRO_HIP_DEBUG_POISON": "7ff80000,mix"})
    _report(case, "poisoned", got, ref)
    _same(got, ref, "poisoned")
    assert got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]


def test_depth_one_and_default_depth_behind_the_sweeps(tmp_path):
    """kTurn90 2304: the persistent launch comes behind the chains of sweeps with ~55 stragglers on a busy device; one twin
    per primary (ALTRO_HIP_TWIN_DEPTH=1, the former rule) and the default depth both equal the launch without twins"""
    case = "turn90_2304"
    ref = _reference(tmp_path, case)
    one = _run(tmp_path, case, "depth1", {"ALTRO_HIP_TWIN_DEPTH": "1"})
    deep = _run(tmp_path, case, "deep", {})
    _report(case, "depth 1", one, ref)
    _report(case, "default", deep, ref)
    _same(one, ref, "depth 1")
    _same(deep, ref, "default depth")
    assert one["tw_"][1] > 0 and one["tw_"][2] == one["tw_"][1], one["tw_"]
    assert deep["tw_"][1] > one["tw_"][1] and deep["tw_"][2] == deep["tw_"][1], deep["tw_"]


@pytest.mark.parametrize("case", ["turn90_16", "turn90_64"])
@pytest.mark.parametrize("k", [1, 2])
def test_refused_joints_leave_the_sequential_result(tmp_path, case, k):
    """No seeded batch breaks a streak early, so no claim is ever wrong.  ALTRO_HIP_TWIN_MISCLAIM=k lets every k-th claim
    assume a regularisation one ulp off: the joint must refuse it, every successor down the chain must drop its column,
    the refusing worker goes on alone -- and the result is still the sequential one."""
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, f"misclaim{k}", {"ALTRO_HIP_TWIN_MISCLAIM": str(k)})
    _report(case, f"misclaim {k}", got, ref)
    _same(got, ref, f"misclaim {k}")
    assert got["tw_"][1] > 0 and got["tw_"][2] < got["tw_"][1], got["tw_"]
