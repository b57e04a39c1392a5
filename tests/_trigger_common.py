"""Shared by the trigger tests (include/altro_trigger.h): the rule stated in numpy, the loop a caller composes from the entry
points, and the pulse disturbances of the closed-loop cases."""
import numpy as np

FIRST, AGE, DEVIATION, VIOLATION, LIMIT, UNSOLVED, AHEAD = 1, 2, 4, 8, 16, 32, 64
SOLVED, UNSOLVED_STATUS = 0, 1  # altro::SolverStatus
N = 24  # horizon of every GPU case


def rule_dict(max_age=1, dx_tol=-1.0, viol_tol=-1.0, on_unsolved=0, lookahead=0, ahead_tol=0.0):
    return dict(max_age=max_age, dx_tol=dx_tol, viol_tol=viol_tol, on_unsolved=on_unsolved, lookahead=lookahead, ahead_tol=ahead_tol)


def reason(rule, B, tracked=None, age=None, status=None, ahead=None):
    """The reason of every instance [B], int32: the OR of the criteria that hold.  tracked / ahead: structured arrays with
    status, violation, max_dx (None: absent); age [B] (None: 0); status [B]: the handle's (None: solved)."""
    age = np.zeros(B, dtype=np.int64) if age is None else np.asarray(age, dtype=np.int64)
    status = np.zeros(B, dtype=np.int64) if status is None else np.asarray(status, dtype=np.int64)
    why = np.zeros(B, dtype=np.int32)
    why[age >= rule["max_age"]] |= AGE
    if tracked is not None:
        with np.errstate(invalid="ignore"):
            if rule["dx_tol"] >= 0:
                why[~(tracked["max_dx"] <= rule["dx_tol"])] |= DEVIATION
            if rule["viol_tol"] >= 0:
                why[~(tracked["violation"] <= rule["viol_tol"])] |= VIOLATION
        why[tracked["status"] != UNSOLVED_STATUS] |= LIMIT
    if rule["on_unsolved"]:
        why[status != SOLVED] |= UNSOLVED
    if rule["lookahead"] > 0 and ahead is not None:
        with np.errstate(invalid="ignore"):
            why[(ahead["status"] != UNSOLVED_STATUS) | ~(ahead["violation"] <= rule["ahead_tol"])] |= AHEAD
    return why


def reason_loop(rule, B, tracked=None, age=None, status=None, ahead=None):
    """reason() as a plain loop over the instances"""
    out = []
    for b in range(B):
        why = 0
        if (0 if age is None else int(age[b])) >= rule["max_age"]:
            why |= AGE
        if tracked is not None:
            if rule["dx_tol"] >= 0 and not float(tracked["max_dx"][b]) <= rule["dx_tol"]:
                why |= DEVIATION
            if rule["viol_tol"] >= 0 and not float(tracked["violation"][b]) <= rule["viol_tol"]:
                why |= VIOLATION
            if int(tracked["status"][b]) != UNSOLVED_STATUS:
                why |= LIMIT
        if rule["on_unsolved"] and (0 if status is None else int(status[b])) != SOLVED:
            why |= UNSOLVED
        if rule["lookahead"] > 0 and ahead is not None and (int(ahead["status"][b]) != UNSOLVED_STATUS
                                                           or not float(ahead["violation"][b]) <= rule["ahead_tol"]):
            why |= AHEAD
        out.append(why)
    return np.asarray(out, dtype=np.int32)


def pulses(cycles, B, shift, n, size, state=1):
    """w [cycles][B][shift][n]: zero for even instances; an odd instance b gets `size` in one state at knot 0 of cycle
    1 + b % 3"""
    w = np.zeros((cycles, B, shift, n))
    for b in range(1, B, 2):
        c = 1 + b % 3
        if c < cycles:
            w[c, b, 0, state] = size
    return w


def composed_loop(s, cycles, shift, rule, w, lo=None, hi=None, snapshot=None):
    """altro_mpc_run_triggered as the caller writes it.  -> the run's dict, plus (with `snapshot`, a function of the handle)
    `around`: per cycle the snapshots before and after the cycle's solve."""
    B, n, m = s.batch, s.n, s.m
    L = cycles * shift
    out = dict(X_cl=np.zeros((B, L + 1, n)), U_cl=np.zeros((B, L, m)), iterations=np.zeros((B, cycles), dtype=np.int32),
               status=np.zeros((B, cycles), dtype=np.int32), reason=np.zeros((B, cycles), dtype=np.int32), masks=[], around=[])
    track = []
    mask = np.ones(B, dtype=bool)
    why = np.full(B, FIRST, dtype=np.int32)
    age = np.zeros(B, dtype=np.int32)
    for c in range(cycles):
        s.set_solve_mask(mask)
        before = snapshot(s) if snapshot else None
        s.solve()
        if snapshot:
            out["around"].append((before, snapshot(s)))
        out["masks"].append(mask.copy())
        age[mask] = 0
        st = s.get_stats()
        out["iterations"][:, c] = np.where(mask, st["iterations_total"], 0)
        out["status"][:, c] = st["status"]
        out["reason"][:, c] = np.where(mask, why, 0)
        t = s.mpc_track(shift, 1, w=None if w is None else w[c][:, None], u_lo=lo, u_hi=hi)
        track.append(t["stats"][:, 0])
        out["X_cl"][:, c * shift:(c + 1) * shift + 1] = t["X_cl"][:, 0]
        out["U_cl"][:, c * shift:(c + 1) * shift] = t["U_cl"][:, 0]
        s.mpc_advance(shift, x0=t["X_cl"][:, 0, shift])
        age += 1
        if c + 1 < cycles:
            mask, why = s.mpc_trigger(rule, tracked=t["stats"][:, 0], age=age, u_lo=lo, u_hi=hi)
    s.set_solve_mask(None)
    out["track"] = np.stack(track, axis=1)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
