"""CPU tier: bench.py's output contract -- the result line stays short whatever the record holds, and --dump-outputs
writes a fixed, bounded sample of what the timed fill left in its arenas."""
import json
from pathlib import Path

import numpy as np

import bench

ROOT = Path(__file__).resolve().parent.parent


def test_result_line_is_short_and_keeps_the_headline():
    for name in ("r06h_bench_default.json", "r06h_bench_n8_folded.json"):
        text = (ROOT / "profiles" / "r06" / name).read_text()
        full = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
        line = bench.result_line(full)
        assert len(json.dumps(line)) < 4096
        for k in ("metric", "value", "unit", "n_gpus", "steps", "ms_per_step", "bit_exact_vs_oracle"):
            assert line[k] == full[k], k
        assert line["roofline"]["frac"] == full["roofline"]["frac"]
        assert [r["kernel_ms"] for r in line["per_rank"]] == [r["kernel_ms"] for r in full["per_rank"]]
        assert {k: c["value"] for k, c in line.get("configs", {}).items()} == {k: c["value"] for k, c in full.get("configs", {}).items()}


class FakeBatch:
    """What dump_outputs reads of a DeviceBatch: the pairs' cell counts and their three int32 matrices."""

    def __init__(self, n, length):
        rng = np.random.default_rng(3)
        self.host = type("H", (), {"n_pairs": n})()
        self.cells_host = np.full(n, (length + 1) ** 2, np.int64)
        self.mats = [tuple(rng.integers(-(1 << 31), 1 << 31, (length + 1) ** 2, dtype=np.int64).astype(np.int32)
                           for _ in range(3)) for _ in range(n)]

    def pair_matrices(self, p):
        return self.mats[p]


def test_dump_outputs_is_a_fixed_exact_bounded_sample(tmp_path):
    db = FakeBatch(1000, 150)
    bench.dump_outputs(tmp_path / "a", db, 0, 0, 1)
    bench.dump_outputs(tmp_path / "b", db, 0, 0, 1)
    for n in ("match", "gap_a", "gap_b", "pair_index", "pair_cells"):
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype == np.float64 and np.array_equal(a, b)
    idx = np.load(tmp_path / "a" / "pair_index.npy").astype(np.int64)
    assert len(idx) == bench.DUMP_MAX_PAIRS and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 1000
    assert np.array_equal(np.load(tmp_path / "a" / "gap_a.npy"), np.concatenate([db.mats[p][1] for p in idx]))

    big = FakeBatch(3, 2000)                          # one pair's matrices alone: 96 MB as float64; rank 1 of 2
    info = bench.dump_outputs(tmp_path / "c", big, 6, 1, 2)
    assert info["bytes"] == sum(p.stat().st_size for p in (tmp_path / "c").iterdir()) <= bench.DUMP_BYTES // 2
    idx = np.load(tmp_path / "c" / "rank1_pair_index.npy")
    m = np.load(tmp_path / "c" / "rank1_match.npy")
    assert len(idx) == 1 and np.array_equal(m, big.mats[int(idx[0]) - 6][0][:len(m)])


def test_plain_run_leaves_every_extra_to_full():
    plain = bench.parse_args(["--gpus", "1", "--steps", "5", "--warmup", "1"])
    assert not plain.full
    assert plain.no_cpu_baseline and plain.no_configs and plain.no_e2e and plain.no_unplaced
    full = bench.parse_args(["--full"])
    assert full.full and not (full.no_cpu_baseline or full.no_configs or full.no_e2e or full.no_unplaced)
    some = bench.parse_args(["--full", "--no-e2e"])
    assert some.no_e2e and not (some.no_cpu_baseline or some.no_configs or some.no_unplaced)


def test_result_line_of_a_plain_record():
    text = (ROOT / "profiles" / "r06" / "r06h_bench_default.json").read_text()
    full = json.loads([l for l in text.splitlines() if l.startswith("{")][-1])
    plain = {k: v for k, v in full.items() if k not in ("bit_exact_vs_oracle", "e2e", "sw_reduce", "configs", "cpu_baseline")}
    line = bench.result_line(plain)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == full[k], k
    assert not {"bit_exact_vs_oracle", "e2e", "sw_reduce", "configs", "cpu_baseline"} & set(line)
