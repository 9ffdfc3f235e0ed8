"""bench.py's plain line and --dump-outputs on the GPU box: a run without --full times exactly --steps steps and prints the headline
fields only (no leg, gate or roofline), and the arrays it dumps are the count table of its last timed step -- here the whole table of a
small workload, compared with the CPU oracle on the same seeded trees (bench.py: seeds 1000 * config + 0 / + 1)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_api import Oracle
from quartetscores_amd import native_ingest, ranks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_line_and_dumped_table_equal_the_oracle(tmp_path):
    n, m, steps = 40, 300, 3
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--taxa", str(n), "--trees", str(m),
                        "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc["metric"] == "quartets counted/sec" and doc["unit"] == "quartets/s" and doc["higher_is_better"] is True
    assert doc["dtype"] == "u32" and doc["steps"] == steps and doc["ms_per_step"] > 0
    assert abs(doc["value"] * doc["ms_per_step"] * 1e-3 / (m * ranks.n_quartets(n)) - 1.0) < 1e-9
    # nothing beside the timed steps: no cpu_baseline / e2e legs, gates, scoring, secondary workloads or roofline
    assert "cpu_baseline" not in doc and "e2e" not in doc and "roofline" not in doc
    cfg = doc["config"]
    assert cfg["parity_tuple_sums_ok"] is None and cfg["score_phase_ms"] is None and cfg["secondary"] is None
    sample = np.load(tmp_path / "count_table_sample.npy")
    index = np.load(tmp_path / "count_table_sample_index.npy")
    sums = np.load(tmp_path / "count_table_cell_sums.npy")
    nq = ranks.n_quartets(n)
    assert sample.dtype == np.float64 and sample.shape == (nq, 3) and (index == np.arange(nq)).all()
    ref_nw = native_ingest.synth_trees(n, 1, 2000).decode().strip()
    text = native_ingest.synth_trees(n, m, 2001).decode().strip()
    o = Oracle(ref_nw)
    o.count(text)
    want = o.counts().astype(np.float64)
    o.close()
    assert (sample == want).all()
    assert (sums == want.sum(axis=0)).all() and sums.sum() == m * nq
