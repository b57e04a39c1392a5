"""Shared by the solve-mask tests (include/altro_subset.h): the ordered compaction per chain slice stated in numpy, the mask
patterns, snapshots of everything a handle lets a caller observe, and the sequential team schedule as a caller composes it."""
import numpy as np

WAVE = 64          # a chain's slice is a whole number of wavefronts
MAX_CHAINS = 4     # chains of batched sweeps of a large batch
CHAINS_FROM = 2048  # ... from this batch size on
N = 24             # horizon of every test problem here


def chain_slices(B, chains=None):
    """[(lo, hi)] of the slices the engine cuts a batch of B into: one below CHAINS_FROM instances, else up to MAX_CHAINS of
    equal size, a whole number of wavefronts each, none of them empty."""
    C = (MAX_CHAINS if B >= CHAINS_FROM else 1) if chains is None else chains
    while True:
        size = -(-(-(-B // C)) // WAVE) * WAVE
        if C == 1 or size * (C - 1) < B:
            break
        C -= 1
    if C == 1:
        return [(0, B)]
    return [(min(B, c * size), min(B, (c + 1) * size)) for c in range(C)]


def compact(mask, slices):
    """(list [B], counts [len(slices)]): the masked-in instances of every slice in ascending order at the slice's own place,
    -1 behind them -- what k_mask_compact writes."""
    mask = np.asarray(mask) != 0
    out = np.full(mask.shape[0], -1, dtype=np.int64)
    counts = np.zeros(len(slices), dtype=np.int64)
    for c, (lo, hi) in enumerate(slices):
        idx = lo + np.flatnonzero(mask[lo:hi])
        out[lo:lo + idx.size] = idx
        counts[c] = idx.size
    return out, counts


def compact_loop(mask, slices):
    """compact() as a plain loop over the instances"""
    out = [-1] * len(mask)
    counts = [0] * len(slices)
    for c, (lo, hi) in enumerate(slices):
        for b in range(lo, hi):
            if mask[b]:
                out[lo + counts[c]] = b
                counts[c] += 1
    return np.asarray(out, dtype=np.int64), np.asarray(counts, dtype=np.int64)


def turn_count(lo, hi, A, a):
    """instances b in [lo, hi) with b % A == a, as the host of a sequential team round knows them without looking"""
    below = lambda x: 0 if x <= a else (x - a - 1) // A + 1  # noqa: E731
    return below(hi) - below(lo)


def patterns(B):
    """name -> mask [B] of the patterns every batch size is run with"""
    idx = np.arange(B)
    out = {"every_other": idx % 2 == 0, "first": idx == 0, "last": idx == B - 1, "ones": np.ones(B, bool), "zeros": np.zeros(B, bool)}
    if len(chain_slices(B)) > 1:
        lo, hi = chain_slices(B)[0]
        out["empty_chain"] = (idx < lo) | (idx >= hi)
        spread = np.zeros(B, bool)
        spread[np.linspace(0, B - 1, 40).astype(int)] = True  # 40 instances over all the slices
        out["spread40"] = spread
    return out


def snapshot(s, history=False):
    """name -> array with the instance as the first axis: everything the handle lets a caller observe"""
    X, U = s.get_trajectory()
    K, d = s.get_gains()
    st = s.get_stats()
    out = dict(X=X, U=U, x0=s.get_initial_state(), duals=s.get_duals(), penalties=s.get_penalties(), cval=s.get_constraint_values(),
               K=np.ascontiguousarray(K), d=d, knot_costs=s.get_knot_costs())
    for name in st.dtype.names:
        out["stats." + name] = np.ascontiguousarray(st[name])
    for k in (0, s.N):
        for key, v in s.get_expansion(k).items():
            # (the terminal knot has no control: altro_get_expansion fills only lxx and lx there and leaves the other
            #  arrays as the caller passed them)
            if k < s.N or key in ("lxx", "lx"):
                out[f"expansion{k}.{key}"] = np.ascontiguousarray(v)
    if history:
        cap = 64
        rows = np.full((s.batch, 2, cap), np.nan)
        for b in range(s.batch):
            for i, field in enumerate(("cost", "alpha")):
                h = s.get_history(b, field, cap)
                rows[b, i, :h.size] = h
        out["history"] = rows
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1)


def differing(a, b, rows):
    """names of the snapshot entries whose bits differ in any of the instances `rows` (a bool mask)"""
    rows = np.asarray(rows, dtype=bool)
    return [k for k in a if not np.array_equal(_bits(a[k])[rows], _bits(b[k])[rows])]


def sequential_loop(s, agents, index, radius, sweeps):
    """altro_team_solve_sequential as the caller writes it; the caller's own mask is put back"""
    before = s.get_solve_mask()
    for _ in range(sweeps):
        for a in range(agents):
            s.team_fill_tracks(agents, index, radius, 0, 1.0)
            s.set_solve_mask(np.arange(s.batch) % agents == a)
            s.solve()
    s.set_solve_mask(None if before.all() else before)
