"""GPU tier: a plain `bench.py --gpus 1` run -- the headline and nothing else.  The extras (oracle spot check, unplaced arenas,
e2e, sw_reduce, configs, cpu_baseline) are --full's; what the plain run dumps is checked against the oracle here instead."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import orclib as O
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def test_plain_bench_run_is_the_headline_only(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[:800]
    res = json.loads(lines[0])
    assert res["metric"] == "dp_cell_updates_per_sec" and res["unit"] == "GCUPS" and res["higher_is_better"] is True
    assert res["dtype"] == "int32" and res["n_gpus"] == 1 and res["steps"] == 20 and res["warmup"] == 2
    assert res["config"]["workload"].startswith("C2") and res["config"]["pairs_per_gpu"] == 10000
    cells = 10000 * 150 * 150
    assert abs(res["value"] - cells / (res["ms_per_step"] * 1e-3) / 1e9) < 1e-6 * res["value"]
    assert res["roofline"]["bound"] == "hbm" and 0 < res["roofline"]["frac"] < 1
    for k in ("bit_exact_vs_oracle", "e2e", "sw_reduce", "configs", "cpu_baseline"):
        assert k not in res, k
    assert "frac_unplaced" not in res["roofline"] and "scale_base" not in res["config"]

    # what the last timed step left in the arenas, for the dumped sample of pairs: the oracle's matrices
    assert res["dump_outputs"]["pairs"] == len(np.load(tmp_path / "pair_index.npy")) > 0
    batch = W.dna_nw_150(10000, seed=1)
    osc = O.Scoring.from_buffer_copy(bytes(S.make_scoring({"preset": "default"})))
    idx = np.load(tmp_path / "pair_index.npy").astype(np.int64)
    counts = np.load(tmp_path / "pair_cells.npy").astype(np.int64)
    got = [np.load(tmp_path / f"{n}.npy") for n in ("match", "gap_a", "gap_b")]
    edges = np.concatenate([[0], np.cumsum(counts)])
    for j in (0, len(idx) // 2, len(idx) - 1):
        p = int(idx[j])
        rc, M, A, B = O.oracle_fill(osc, batch.seq_a(p), batch.seq_b(p), 0)
        assert rc == 0 and counts[j] == M.size, p
        for g, want in zip(got, (M, A, B)):
            assert np.array_equal(g[edges[j]:edges[j + 1]], want.astype(np.float64)), p
