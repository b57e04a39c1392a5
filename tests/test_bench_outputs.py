"""bench.py's plain run and `--dump-outputs DIR`.

CPU: dump_outputs() on an oracle-backed solver -- the records and trajectories land as float64 .npy files, and past the
size limit the trajectories are cut to a fixed seeded sample of instances.  GPU: a plain run prints the headline alone
(the blocks of `--full` are absent), the dump holds the last timed step's results, and two runs with the same arguments
dump the same bits."""
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "cpu_baseline", "host_boundary", "other_configs", "latency", "fast_forward", "pipeline_2", "device_loop")


def _oracle_solved(A, P, oracle_make, batch):
    o = P.batch_turn90(oracle_make, batch=batch, dtype=A.F64, seed=P.SEED_BASE + 3)
    o.solve()
    return o


def test_dump_outputs_writes_records_and_trajectories(A, P, S, oracle_make, tmp_path):
    bench = importlib.import_module("bench")
    o = _oracle_solved(A, P, oracle_make, 6)
    rec = S.result_records(o.get_stats())
    names = bench.dump_outputs(str(tmp_path), rec, o)
    assert names == ["U", "X", "records"]
    X, U = o.get_trajectory()
    for name, want in (("records", rec), ("X", X), ("U", U)):
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want), name


def test_dump_outputs_samples_past_the_limit(A, P, S, oracle_make, tmp_path, monkeypatch):
    bench = importlib.import_module("bench")
    o = _oracle_solved(A, P, oracle_make, 10)
    rec = S.result_records(o.get_stats())
    X, U = o.get_trajectory()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", rec.nbytes + 3 * (X[0].nbytes + U[0].nbytes))
    for d in ("a", "b"):
        assert bench.dump_outputs(str(tmp_path / d), rec, o) == ["U", "X", "instances", "records"]
    idx = np.load(tmp_path / "a" / "instances.npy")
    assert idx.dtype == np.float64 and len(idx) == 3 and (np.diff(idx) > 0).all()
    assert np.array_equal(idx, np.load(tmp_path / "b" / "instances.npy"))  # a fixed sample
    i = idx.astype(int)
    assert np.array_equal(np.load(tmp_path / "a" / "X.npy"), X[i]) and np.array_equal(np.load(tmp_path / "a" / "U.npy"), U[i])
    assert np.array_equal(np.load(tmp_path / "a" / "records.npy"), rec)  # the records are always whole
    total = sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a"))  # (128 B .npy headers)
    assert total <= bench.DUMP_LIMIT_BYTES + idx.nbytes


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "256",
               "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    line = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert not [k for k in FULL_ONLY if k in line]
    rec = np.load(tmp_path / "a" / "records.npy")
    X, U = np.load(tmp_path / "a" / "X.npy"), np.load(tmp_path / "a" / "U.npy")
    assert rec.shape == (256, 4) and X.shape == (256, 101, 3) and U.shape == (256, 100, 2)
    assert rec.dtype == X.dtype == U.dtype == np.float64
    # the records are those the line was computed from: {cost, violation, iterations_total, status}
    assert round(float((rec[:, 3] == 0).mean()), 5) == line["config"]["solved_fraction"]
    assert int(rec[:, 2].max()) == line["config"]["max_iterations"]
    # seeded inputs: the same arguments give the same results
    for name in ("records", "X", "U"):
        assert np.array_equal(np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))), name
