"""GPU tier: a plain bench.py run (set-up, warm-up, the timed steps, the headline line) and what --dump-outputs writes: the per-read
records of the last timed step for a fixed sample of the reads, the same in every run with the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _bench(tmp_path, tag, steps):
    out, hits = tmp_path / ("out_" + tag), tmp_path / ("hits_" + tag)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--genome-mbp", "8", "--contigs", "4", "--reads", "250000", "--dump-outputs", str(out), "--dump-hits", str(hits)]
    r = subprocess.run(cmd, timeout=600, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.split("\n") if l.startswith("{")]
    assert len(line) == 1
    return json.loads(line[0]), out, np.load(str(hits / "hits_rank0.npy"))


def test_plain_run_and_dump_outputs(tmp_path):
    d, out, hits = _bench(tmp_path, "a", 3)
    assert (d["steps"], d["warmup"], d["n_gpus"], d["unit"], d["higher_is_better"], d["dtype"]) == (3, 1, 1, "reads/s", True, "u64")
    assert abs(d["value"] - 250000 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert not {"roofline", "kstats", "drain", "cpu_baseline", "parity_sample", "t_e2e_s"} & set(d)      # those take --full
    idx = np.load(str(out / "read_index.npy"))
    assert idx.dtype == np.float64 and len(idx) == 200000 and np.all(np.diff(idx) > 0) and idx[-1] < 250000
    rows = idx.astype(np.int64)
    total = idx.nbytes
    for f in hits.dtype.names:
        a = np.load(str(out / (f + ".npy")))
        assert a.dtype == np.float64 and np.array_equal(a, hits[f][rows].astype(np.float64)), f
        total += a.nbytes
    assert total <= 64 << 20
    assert (hits["type"][rows] != 0).mean() > 0.8
    # same arguments but the step count: the same reads are sampled and the last step computed the same records
    d2, out2, _ = _bench(tmp_path, "b", 2)
    assert d2["steps"] == 2
    assert sorted(os.listdir(str(out2))) == sorted(os.listdir(str(out)))
    for name in os.listdir(str(out)):
        assert np.array_equal(np.load(str(out / name)), np.load(str(out2 / name))), name
