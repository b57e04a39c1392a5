"""The sequential (Gauss-Seidel) team schedule of include/altro_subset.h composed by the caller on the CPU ORACLE.  Needs no GPU.
The oracle has no mask, but its instances are independent: every turn builds a FRESH handle from
problems.team_ring(per_knot_track = the rows everyone's current plans give, U = the current controls), solves it, and takes
over only the rows of the turn's agents (b % A == a) -- which is what "masked" means.  The clearances are in DISTANCE units,
min(|p_a - p_j| - R) over knots 1 .. N - 1 and all pairs.

ONE sweep from the uncoupled plans is what the bars are about.  (A second sweep from a cold AL start at T = 2, A = 5 leaves one
instance at ALTRO_MAX_INNER_ITERATIONS on the oracle itself: the problem's behaviour, not the schedule's.)

With ALTRO_WRITE_PROFILES=1 the measured values go to profiles/subset_oracle_clearance.json."""
import json
import os

import numpy as np
import pytest

import _team_common as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
CASES = [(3, 2), (2, 3), (2, 5)]
_MEASURED = {}


def sequential_sweep(P, make, teams, agents, X, U, stats, rad):
    """one sweep: agent 0 of every team re-plans against everyone's current plan, then agent 1, ...; returns X, U, stats"""
    B = teams * agents
    X, U, stats = X.copy(), U.copy(), stats.copy()
    for a in range(agents):
        turn = np.arange(B) % agents == a
        s = P.team_ring(make, teams, agents, N=N, per_knot_track=TC.fill_rows(X, agents, rad, TC.ALL), U=U)
        s.solve()
        Xn, Un = s.get_trajectory()
        sn = s.get_stats()
        s.close()
        X[turn], U[turn], stats[turn] = Xn[turn], Un[turn], sn[turn]
    return X, U, stats


@pytest.mark.parametrize("teams,agents", CASES)
def test_one_sequential_sweep_settles_the_ring(A, P, oracle_make, teams, agents):
    s = P.team_ring(oracle_make, teams, agents, N=N, per_knot_track=np.zeros((teams * agents, N + 1, 3 * (agents - 1))))
    s.solve()
    X, U = s.get_trajectory()
    stats = s.get_stats()
    rad = s.team_radius
    s.close()
    unc = TC.distance_clearance(X, agents, rad, 1, N)
    X, U, stats = sequential_sweep(P, oracle_make, teams, agents, X, U, stats, rad)
    cpl = TC.distance_clearance(X, agents, rad, 1, N)
    print(f"T {teams} A {agents}: uncoupled {unc}, after one sequential sweep {cpl}, statuses {np.unique(stats['status'])}, "
          f"iterations {stats['iterations_total'].tolist()}")
    _MEASURED[f"sequential_T{teams}_A{agents}"] = dict(uncoupled=unc.tolist(), one_sweep=cpl.tolist(),
                                                       iterations=stats["iterations_total"].tolist())
    assert (unc <= TC.UNCOUPLED_BAR).all(), unc
    assert (stats["status"] == A.SOLVED).all(), stats["status"]
    assert (cpl >= TC.COUPLED_BAR).all(), cpl


def test_measured_values_are_recorded():
    """profiles/subset_oracle_clearance.json holds a value for every case above (written with ALTRO_WRITE_PROFILES=1)."""
    path = os.path.join(ROOT, "profiles", "subset_oracle_clearance.json")
    if os.environ.get("ALTRO_WRITE_PROFILES") == "1" and _MEASURED:
        with open(path, "w") as f:
            json.dump(dict(units="distance: min(|p_a - p_j| - R) over knots 1 .. N - 1, N = 24; per team", **_MEASURED), f, indent=1)
    rec = json.load(open(path))
    for teams, agents in CASES:
        assert f"sequential_T{teams}_A{agents}" in rec
