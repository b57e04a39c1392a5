# One GPU visit: parity tests, smoke, bench, rocprof kernel trace of the bench.
cd $GRAFT_REPO_ROOT
OUT=${OUT:-results}  # (where the logs and the trace go)
mkdir -p "$OUT"
export TMPDIR=/tmp
python -m pytest tests -q -m gpu 2>&1 | grep -v "^E  " | tail -12 | tee "$OUT/pytest_gpu.log"
python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 | tee "$OUT/smoke.log"
python bench.py --steps 3 --warmup 1 --full 2>&1 | tail -1 | tee "$OUT/bench.log"
rm -rf "$OUT/prof"
rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o bench -- python bench.py --steps 1 --warmup 0 --full --no-cpu-baseline > "$OUT/prof_run.log" 2>&1
python - "$OUT" <<'PY'
import csv, glob, collections, sys
f = glob.glob(sys.argv[1] + '/prof/**/*kernel_trace.csv', recursive=True)[0]
rows = list(csv.DictReader(open(f)))
per = collections.defaultdict(list)
for r in rows:
    name = r['Kernel_Name']
    short = 'fwd' if 'k_forward' in name else 'bwd' if 'k_backward' in name else 'exp' if 'k_expansions' in name else None
    if short: per[short].append((int(r['Start_Timestamp']), (int(r['End_Timestamp'])-int(r['Start_Timestamp']))/1e3))
for k,v in per.items():
    v.sort()
    d=[x[1] for x in v]
    n=len(d)//2
    print(k, 'launches', len(d), 'first solve durations us:', [round(x) for x in d[:n][:20]], '...', [round(x) for x in d[:n][-6:]])
PY
