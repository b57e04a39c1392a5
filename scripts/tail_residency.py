"""Who is resident in the persistent tail launch (k_sweep_fused), by 100 us and by XCD, from the mailbox dump.

  ALTRO_HIP_TWIN_DEBUG=all [ALTRO_HIP_TAIL_WORKERS=0] python scripts/tail_residency.py run [batch] 2> dump.txt
  python scripts/tail_residency.py table dump.txt

`run` is the probe of profiles/tail_endgame_experiments.txt: batch_turn90 of the given batch (4096: the headline's problem)
with seed SEED_BASE + 3, three solves through one handle; the library prints the dump of every solve to stderr.  `table`
reads the LAST solve's dump.  A job is a primary slot or a pool slot; its line carries the XCD it ran on and the physical
workgroup (`worker`) that ran it.  On the one-shot grid a job is a workgroup, so "jobs resident" is "workgroups resident";
on the worker grid the workers are resident for the whole launch and the table shows how many of them have a job."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(batch):
    import importlib
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    A = g.load_package()
    P = importlib.import_module("altro_cpp_amd.problems")
    s = P.batch_turn90(lambda n, m, N, b, d: A.BatchSolver(n, m, N, b, d), batch=batch, seed=P.SEED_BASE + 3)
    for rep in range(3):
        s.reset_trajectory()
        s.solve()
        tm = s.get_timing()
        print(f"solve {rep}: total_ms {tm['total_ms']:.3f} pool {tm['twin_workgroups']} claims {tm['twin_claims']} "
              f"joints {tm['twin_handovers']} most iterations of one job {tm['fused_workgroup_iterations']}")
    s.close()


def _num(line, key):
    m = re.search(r"\b" + key + r" (-?\d+)", line)
    return int(m.group(1)) if m else -1


def table(path):
    lines = open(path, errors="replace").read().split("\n")
    ends = [i for i, l in enumerate(lines) if l.startswith("twin mailboxes:")]
    if not ends:
        sys.exit("no mailbox dump in " + path)
    first = ends[-2] + 1 if len(ends) > 1 else 0
    jobs = []   # (kind, looking from, working from, until, xcd, worker)
    for l in lines[first:ends[-1]]:
        l = l.strip()
        xcd, worker = _num(l, "xcd"), _num(l, "worker")
        if l.startswith("primary"):
            t0, t1 = _num(l, "start"), max(_num(l, "handed"), _num(l, "end"))
            jobs.append(("primary", t0, t0, t1, xcd, worker))
        elif l.startswith("segment"):
            t1 = max(_num(l, k) for k in ("done", "verdict", "handed", "commit", "cloned", "go"))
            jobs.append(("segment", _num(l, "start"), _num(l, "go"), t1, xcd, worker))
        elif l.startswith("idle"):
            jobs.append(("idle", _num(l, "start"), 1 << 30, _num(l, "left"), xcd, worker))
    jobs = [j for j in jobs if j[1] >= 0 and j[3] >= j[1]]
    last = max(j[3] for j in jobs)
    workers = sorted({j[5] for j in jobs if j[5] >= 0})
    left = {w: max(j[3] for j in jobs if j[5] == w) for w in workers}   # (a worker is resident until its last job ends)
    nx = max([j[4] for j in jobs] + [0]) + 1
    print(lines[ends[-1] - 1])
    print(lines[ends[-1]])
    print(f"{len(jobs)} jobs on {len(workers)} physical workgroups; last job ends at {last} us")
    print("     t   primaries  segments  looking   jobs | by XCD " + " ".join(f"{x:4d}" for x in range(nx)) + " | workgroups with a job / still resident")
    for t in range(0, last + 100, 100):
        on = [j for j in jobs if j[1] <= t < j[3]]
        prim = sum(1 for j in on if j[0] == "primary")
        seg = sum(1 for j in on if j[0] == "segment" and j[2] <= t)
        look = len(on) - prim - seg
        by = [sum(1 for j in on if j[4] == x) for x in range(nx)]
        busy = len({j[5] for j in on if j[5] >= 0 and not (j[0] != "primary" and j[2] > t)})
        res = sum(1 for w in workers if left[w] > t)
        print(f"{t:6d}   {prim:9d} {seg:9d} {look:8d} {len(on):6d} |        " + " ".join(f"{n:4d}" for n in by) + f" | {busy:4d} / {res:4d}")
    starts = sorted(j[1] for j in jobs)
    print("job starts per 100 us: " + " ".join(str(sum(1 for s in starts if t <= s < t + 100)) for t in range(0, last + 100, 100)))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run(int(sys.argv[2]) if len(sys.argv) > 2 else 4096)
    elif len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
