"""The worker grid of the persistent tail (TwinCtl::workers, k_sweep_fused): the launch has as many workgroups as the
device holds at once, and each takes the launch's jobs -- primary slots, then pool slots -- by ticket
(ALTRO_HIP_TAIL_WORKERS: unset = resident workers, 0 = the one-shot grid with a workgroup per job, n = at most n workers).

Which physical workgroup plays which block may not change a result.  Each case is compared with a launch without twins
(ALTRO_HIP_TWIN=0, always the one-shot grid) bit for bit: trajectories, gains, multipliers, penalties, stored constraint
values, expansion records, knot costs, every statistic.  What is new is REUSE -- one workgroup runs several jobs, so LDS,
sequence words or a mailbox of the job before could leak into the next -- and a few workers force it: 8 workers on a batch
of 64 run several primaries each and then several claims, one worker on a batch of 16 walks every primary and must then
end the launch by the pool's rule, since no claim can ever be served.  Every run is two solves through one handle in a
fresh child process (the switches are read once per process)."""
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
case, path = sys.argv[1], sys.argv[2]
cases = {"turn90_16": lambda: P.batch_turn90(make, batch=16, seed=P.SEED_BASE + 3),
         "turn90_64": lambda: P.batch_turn90(make, batch=64, seed=P.SEED_BASE + 3),
         "obstacles_48": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F64),
         "obstacles_48_r32": lambda: P.batch_three_obstacles(make, batch=48, dtype=A.F32)}   # fp32 records: the SEG-capable variant
s = cases[case]()
for rep in range(2):   # (the second solve reuses mailboxes, shadow columns and ticket counters)
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
out["tw_"] = np.array([tm["twin_workgroups"], tm["twin_claims"], tm["twin_handovers"], tm["fused_workgroup_iterations"]])
out["ms_"] = np.array([tm["total_ms"]])
s.close()
np.savez(path, **out)
'''

CASES = ["turn90_16", "turn90_64", "obstacles_48", "obstacles_48_r32"]
_SWITCHES = ("ALTRO_HIP_TWIN", "ALTRO_HIP_TWIN_MIN", "ALTRO_HIP_TWIN_DEPTH", "ALTRO_HIP_TWIN_MISCLAIM", "ALTRO_HIP_DEBUG_POISON",
             "ALTRO_HIP_TAIL_WORKERS", "ALTRO_HIP_TWIN_DEBUG")
_solo = {}
# the two combinations that force reuse: (case, workers)
FEW = [("turn90_64", "8"), ("turn90_16", "1")]
VARIANTS = {"plain": {},
            "poisoned": {"ALTRO_HIP_DEBUG_POISON": "7ff80000,mix"},
            "floor_depth5": {"ALTRO_HIP_TWIN_MIN": "3", "ALTRO_HIP_TWIN_DEPTH": "5"},
            "misclaim1": {"ALTRO_HIP_TWIN_MISCLAIM": "1"},
            "misclaim2": {"ALTRO_HIP_TWIN_MISCLAIM": "2"}}


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
        if k.endswith("_"):   # (pool size, claims, joints, a job's iterations, milliseconds)
            continue
        assert np.array_equal(got[k], ref[k]), (what, k, np.abs(np.asarray(got[k], float) - np.asarray(ref[k], float)).max())


def _report(case, tag, got, ref):
    print(f"{case} [{tag}]: pool / claims / confirmed joints / most iterations of one job {got['tw_'].tolist()}, "
          f"ms {got['ms_'][0]:.3f} (without twins {ref['ms_'][0]:.3f}, {int(ref['tw_'][3])} iterations)")


@pytest.mark.parametrize("case", CASES)
def test_worker_grid_and_one_shot_grid_are_bit_identical(tmp_path, case):
    ref = _reference(tmp_path, case)
    workers = _run(tmp_path, case, "default", {})
    one_shot = _run(tmp_path, case, "one_shot", {"ALTRO_HIP_TAIL_WORKERS": "0"})
    _report(case, "default", workers, ref)
    _report(case, "one-shot grid", one_shot, ref)
    _same(workers, ref, "default")
    _same(one_shot, ref, "one-shot grid")
    for got in (workers, one_shot):
        # the pool's size is the number of pool tickets, whatever the grid; no streak of these batches breaks before the
        # iteration cap: every claim is confirmed at its joint
        assert got["tw_"][0] == workers["tw_"][0] > 0 and got["tw_"][1] > 0 and got["tw_"][2] == got["tw_"][1], got["tw_"]
        # "most iterations of one job" stays a job's figure: a split streak's longest share, never a worker's sum over its jobs
        assert 0 < got["tw_"][3] <= ref["tw_"][3], (got["tw_"], ref["tw_"])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("case,n", FEW)
def test_few_workers_reuse_everything(tmp_path, case, n, variant):
    ref = _reference(tmp_path, case)
    got = _run(tmp_path, case, f"workers{n}_{variant}", dict(VARIANTS[variant], ALTRO_HIP_TAIL_WORKERS=n))
    _report(case, f"{n} workers, {variant}", got, ref)
    _same(got, ref, f"{n} workers, {variant}")
    pool, claims, joints, job_loops = (int(v) for v in got["tw_"])
    assert pool > 0
    if n == "1":
        # one worker: every primary has finished before the first pool ticket is taken -- nothing to claim, the pool job
        # sees that nobody can publish any more and the launch ends; the straggler walked its streak alone
        assert claims == 0 and joints == 0 and job_loops == int(ref["tw_"][3]), got["tw_"]
    else:
        # eight workers: the stragglers outlive the primary tickets, so the workers that run out of primaries serve claims
        assert claims > 0 and 0 < job_loops <= int(ref["tw_"][3]), got["tw_"]
        if variant.startswith("misclaim"):
            assert joints < claims, got["tw_"]   # (a claim one ulp off is refused at its joint, and its line with it)
        else:
            assert joints == claims, got["tw_"]
