"""bench.py command line: --dump-outputs writes the last timed step's
result, a plain run leaves the extra checks to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def test_dump_outputs_dtypes_and_values(tmp_path):
    rng = np.random.default_rng(0)
    dists = rng.random((37, 10), dtype=np.float32)
    ids = rng.integers(0, 10_000_000, size=(37, 10)).astype(np.int64)
    ids[3, 7:] = -1  # unfilled slots
    bench.dump_outputs(str(tmp_path / "o"), dists, ids)
    d = np.load(tmp_path / "o" / "dists.npy")
    i = np.load(tmp_path / "o" / "ids.npy")
    assert d.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(d, dists)
    assert np.array_equal(i.astype(np.int64), ids)
    assert not (tmp_path / "o" / "rows.npy").exists()


def test_dump_outputs_samples_above_the_size_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    k = 10
    dists = np.arange(1000 * k, dtype=np.float32).reshape(1000, k)
    ids = np.arange(1000 * k, dtype=np.int64).reshape(1000, k)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), dists, ids)
    a = {f: np.load(tmp_path / "a" / f"{f}.npy")
         for f in ("dists", "ids", "rows")}
    b = {f: np.load(tmp_path / "b" / f"{f}.npy")
         for f in ("dists", "ids", "rows")}
    assert sum(v.nbytes for v in a.values()) <= 4096
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < 1000 and len(np.unique(rows)) == len(rows)
    assert np.array_equal(a["dists"], dists[rows])
    assert np.array_equal(a["ids"].astype(np.int64), ids[rows])
    for f in a:  # the sample is fixed: same rows on every run
        assert np.array_equal(a[f], b[f])


def test_gen_data_chunks_match_gen_data():
    """The streamed setup must feed the engine the table gen_data makes."""
    ref = bench.gen_data(2500, 8, seed=42, ncl=16, chunk=1000)
    out = np.empty((2500, 8), dtype=np.float32)
    spans = list(bench.gen_data_chunks(out, seed=42, ncl=16, chunk=1000))
    assert spans == [(0, 1000), (1000, 2000), (2000, 2500)]
    assert np.array_equal(out, ref)


@pytest.mark.gpu
def test_plain_run_dumps_last_step_and_skips_the_extras(tmp_path):
    out = tmp_path / "dump"
    nq, steps = 64, 3
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
           "--steps", str(steps), "--warmup", "1", "--db-size", "20000",
           "--nlist", "64", "--queries", str(nq),
           "--dump-outputs", str(out)]
    p = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert line["unit"] == "QPS" and line["higher_is_better"] is True
    assert line["dtype"] == "f32"
    assert abs(line["value"] - nq / (line["ms_per_step"] / 1000.0)) \
        <= 0.01 * line["value"]
    # what moved behind --full is absent from a plain run
    assert line["cpu_baseline"] is None
    assert line["config"]["recall_at_10"] is None
    assert line["config"]["scanned_codes_per_query"] is None
    d = np.load(out / "dists.npy")
    i = np.load(out / "ids.npy")
    assert d.dtype == np.float32 and i.dtype == np.float64
    assert d.shape == (nq, 10) and i.shape == (nq, 10)
    # queries are perturbed DB rows: every query finds k real neighbours,
    # nearest first
    assert (i >= 0).all() and (i < 20000).all()
    assert np.array_equal(i, np.round(i))
    assert (np.diff(d, axis=1) >= 0).all()
