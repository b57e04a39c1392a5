"""The plan exchange of include/altro_team.h composed by the caller on the CPU ORACLE (tests/_team_common.host_exchange: a
fresh handle per round from problems.team_ring(per_knot_track=...), one ordinary circle constraint per knot).  Needs no GPU.
It pins the conditions tests/test_team_gpu.py relies on: the uncoupled plans collide, plain simultaneous exchange
oscillates, and the damped and the prioritised exchange both settle.  The clearances here are in DISTANCE units,
min(|p_a - p_j| - R) over knots 1 .. N - 1 and all pairs.

With ALTRO_WRITE_PROFILES=1 the measured values go to profiles/team_oracle_clearance.json."""
import json
import os

import numpy as np
import pytest

import _team_common as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 24
_MEASURED = {}


@pytest.mark.parametrize("teams,agents", [(3, 2), (2, 3), (2, 5)])
def test_uncoupled_plans_collide(A, P, oracle_make, teams, agents):
    log = []
    _, _, stats = TC.host_exchange(P, oracle_make, teams, agents, TC.ALL, 1.0, 0, N=N, log=log)
    print(f"uncoupled T {teams} A {agents}: clearance {log[0]}, statuses {np.unique(stats['status'])}")
    _MEASURED[f"uncoupled_T{teams}_A{agents}"] = log[0].tolist()
    assert (stats["status"] == A.SOLVED).all()
    assert (log[0] <= TC.UNCOUPLED_BAR).all(), log[0]


def test_plain_exchange_oscillates(A, P, oracle_make):
    """ALTRO_TEAM_ALL with blend = 1: both agents dodge, then both see the other has dodged and go straight again.  Why the
    blend exists."""
    log = []
    TC.host_exchange(P, oracle_make, 3, 2, TC.ALL, 1.0, 6, N=N, log=log)
    rounds = np.array(log[1:])  # [6][T]
    print("plain exchange, clearance per round and team:\n", rounds)
    _MEASURED["plain_exchange_T3_A2"] = rounds.tolist()
    assert (np.sign(rounds[1:]) == -np.sign(rounds[:-1])).all() and (rounds != 0).all(), rounds


@pytest.mark.parametrize("case", TC.CASES, ids=TC.case_id)
def test_damped_and_priority_exchange_settle(A, P, oracle_make, case):
    """Every instance ALTRO_SOLVED and clearance >= -2e-3 after the case's rounds.  The bar: the AL stops at c <= 1e-4 against
    LAST round's plans and the peers still move by up to 3e-3 between rounds; measured worst cases are written to
    profiles/team_oracle_clearance.json."""
    teams, agents, mode, blend, rounds = case
    log = []
    _, _, stats = TC.host_exchange(P, oracle_make, teams, agents, mode, blend, rounds, N=N, log=log)
    print(f"{TC.case_id(case)}: clearance per round (min over teams) {[float(x.min()) for x in log]}")
    _MEASURED[TC.case_id(case)] = [x.tolist() for x in log]
    assert (stats["status"] == A.SOLVED).all(), stats["status"]
    assert (log[-1] >= TC.COUPLED_BAR).all(), log[-1]


def test_measured_values_are_recorded():
    """profiles/team_oracle_clearance.json holds a value for every case above (written with ALTRO_WRITE_PROFILES=1)."""
    path = os.path.join(ROOT, "profiles", "team_oracle_clearance.json")
    if os.environ.get("ALTRO_WRITE_PROFILES") == "1" and _MEASURED:
        with open(path, "w") as f:
            json.dump(dict(units="distance: min(|p_a - p_j| - R) over knots 1 .. N - 1, N = 24; per round, per team",
                           **_MEASURED), f, indent=1)
    rec = json.load(open(path))
    for case in TC.CASES:
        assert TC.case_id(case) in rec
    assert "plain_exchange_T3_A2" in rec and "uncoupled_T2_A5" in rec
