#!/usr/bin/env python3
"""align_banded_sw_bench.py -- banded SW (seqalign_sw_score_banded / seqalign_sw_align_banded) against the unbanded calls, in
one process.

Workloads (seeded; the band is the read's true offset in its window +- w, as a seed or an index would give it):
  W1   10 000 reads of 700 bp in 1 000 bp windows (README's workload: dna_sw_read_vs_ref, seed 2), w = 32
  W2   1 000 reads of 10 kb with 8 % edits (equal thirds) in 12 kb windows, w = 256
  W3   C3's batch (bench.py, tests/golden/configs.json "C3": 10 000 reads of 150 bp in 1 000 bp windows), w = 16
  each: sw_align_banded against sw_batch(max_hits = 1), sw_score_banded against sw_score; scoring 2 / -2 / -2 / -1 (C3's)
  F    frame rate, kernel time against kernel time (HIP events around the launches, sequences already on the device):
       seqalign_sw_band_score_time_ms on pairs whose band fills a frame (64 x CPL diagonals) beside seqalign_score_time_ms
       (SW) on pairs as wide as that frame (len_a = 64 x CPL), same rows -- cells of the frame per second

One JSON line per workload: median wall clock of 3 synchronous calls after a warm-up (the align calls raw: no Python dict
per hit on either side).  Before a line is printed the tool
ASSERTS that the banded hit equals sw_batch's, field for field, for every pair whose unbanded walk lies in its band (in_band
counts them), that no banded score is above the unbanded one and that the score call agrees with the align call; it exits
non-zero otherwise.  W2 carries `bar_met`: both banded calls took less than half their unbanded counterpart's time (a line
with bar_met false is flagged on stderr and the exit status is 2); W1 and W3 are recorded without a bar.  --scale divides the
pair counts (a quick run).

    python seq-align_amd/tools/align_banded_sw_bench.py [--only W1,W2,W3,F] [--scale 1] [--calls 3] [--warm 1]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "seq-align_amd" / "tools")]

import seqalign_amd as S                      # noqa: E402
from seqalign_amd import workloads as W       # noqa: E402
from align_banded_bench import median_ms, related   # noqa: E402

SW_SPEC = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def read_vs_ref(n, read_len, ref_len=1000, seed=2):
    """workloads.dna_sw_read_vs_ref and the offsets it drew: the same two draws from the same generator"""
    rng = W.Rng(seed)
    rng.below(4, n * ref_len)
    start = rng.below(ref_len - read_len - 8, n).astype(np.int64)
    return W.dna_sw_read_vs_ref(n, seed=seed, read_len=read_len, ref_len=ref_len), start


def workload(name, scale):
    if name == "W1":
        batch, start = read_vs_ref(max(1, 10_000 // scale), 700)
        return batch, start, 32
    if name == "W3":
        batch, start = read_vs_ref(max(1, 10_000 // scale), 150)
        return batch, start, 16
    rng = W.Rng(1400)
    pairs, start = [], []
    for _ in range(max(1, 1000 // scale)):
        window = ACGT[rng.below(4, 12_000).astype(np.int64)].tobytes()
        off = int(rng.below(2000, 1)[0])
        src, read = related(rng, 10_000, 0.08)
        # the read is an edited copy of the window's stretch: plant the unedited source there
        window = window[:off] + src + window[off + len(src):]
        pairs.append((read, window))
        start.append(off)
    return W.from_pairs(pairs), np.asarray(start, np.int64), 256


def excursion(hit):
    """(lowest, highest) i - j over the cells of a hit's walk, start and end cell included"""
    x = np.frombuffer(hit["a"].encode(), np.uint8) != 0x2D
    y = np.frombuffer(hit["b"].encode(), np.uint8) != 0x2D
    d = hit["pos_a"] - hit["pos_b"] + np.concatenate(([0], np.cumsum(x.astype(np.int64) - y.astype(np.int64))))
    return int(d.min()), int(d.max())


def run_workload(ctx, sc, name, args):
    batch, start, w = workload(name, args.scale)
    n = batch.n_pairs
    lo, hi = (-start - w).astype(np.int32), (-start + w).astype(np.int32)
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    d_lo, d_hi = np.maximum(lo, -lbs), np.minimum(hi, las)
    rows = np.maximum(0, np.minimum(lbs, las - d_lo) - np.maximum(1, 1 - d_hi) + 1)
    band_cells = int((rows * (d_hi - d_lo + 1)).sum())
    cells = int((las * lbs).sum())
    out = {"workload": name, "pairs": n, "w": w, "max_width": int((d_hi - d_lo + 1).max()), "cells": cells, "band_cells": band_cells,
           "cell_ratio": round(cells / band_cells, 1)}
    ms, all_ = median_ms(lambda: ctx.sw_align_banded(batch, sc, lo, hi, 1, raw=True), args.calls, args.warm)
    got = ctx.sw_align_banded(batch, sc, lo, hi, 1)
    out.update(align_banded_ms=round(ms, 2), align_banded_all=all_, align_launches=ctx.last_call())
    ms_b, all_b = median_ms(lambda: ctx.sw_batch(batch, sc, 1, max_hits=1, raw=True), args.calls, args.warm)
    want = ctx.sw_batch(batch, sc, 1, max_hits=1)
    out.update(align_base="sw_batch(max_hits=1)", align_base_ms=round(ms_b, 2), align_base_all=all_b, align_base_launches=ctx.last_call(),
               align_speedup=round(ms_b / ms, 2))
    inside = []
    for p in range(n):
        if not want[p]:
            inside.append(True)                       # no cell above 0 anywhere: none in the band either
            continue
        e_lo, e_hi = excursion(want[p][0])
        inside.append(int(lo[p]) <= e_lo and e_hi <= int(hi[p]))
    wrong = [p for p in range(n) if inside[p] and got[p] != want[p]]
    assert not wrong, (name, "banded hit differs from sw_batch's although its walk lies in the band", wrong[:5])
    score_of = lambda hits: hits[0]["score"] if hits else 0
    above = [p for p in range(n) if score_of(got[p]) > score_of(want[p])]
    assert not above, (name, "banded score above the unbanded one", above[:5])
    out.update(in_band=int(sum(inside)), identical=True, outside_not_above=True)
    ms, all_ = median_ms(lambda: ctx.sw_score_banded(batch, sc, lo, hi), args.calls, args.warm)
    ms_b, all_b = median_ms(lambda: ctx.sw_score(batch, sc), args.calls, args.warm)
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    ends = [(h[0]["score"], h[0]["pos_a"] + h[0]["len_a"], h[0]["pos_b"] + h[0]["len_b"]) if h else (0, 0, 0) for h in got]
    assert [(int(s), int(x), int(y)) for s, x, y in zip(score, end_a, end_b)] == ends, (name, "the score call disagrees with the align call")
    out.update(score_banded_ms=round(ms, 2), score_banded_all=all_, score_launches=ctx.last_call(), score_base="sw_score",
               score_base_ms=round(ms_b, 2), score_base_all=all_b, score_speedup=round(ms_b / ms, 2), score_equals_align=True)
    ok = True
    if name == "W2":
        ok = out["align_speedup"] > 2 and out["score_speedup"] > 2
        out["bar_met"] = ok
    print(json.dumps(out), flush=True)
    if not ok:
        print(f"{name}: BAR MISSED: align {out['align_speedup']}x, score {out['score_speedup']}x", file=sys.stderr, flush=True)
    return ok


def run_frame_rate(ctx, sc, args):
    rows, pairs = 4000, max(64, 4096 // args.scale)
    rng = W.Rng(77)
    for cpl in (1, 2, 4, 8, 16):
        frame = 64 * cpl
        seqs = [related(rng, rows, 0.02) for _ in range(8)]
        batch = W.from_pairs([(seqs[k % 8][0], seqs[k % 8][0]) for k in range(pairs)])
        lo = -(frame // 2)
        band_ms = float(np.median(ctx.sw_band_score_time_ms(batch, sc, lo, lo + frame - 1, repeats=5)))
        wide = W.from_pairs([(seqs[k % 8][0][:frame], seqs[k % 8][1][:rows]) for k in range(pairs)])
        full_ms = float(np.median(ctx.score_time_ms(wide, sc, 1, repeats=5)))
        band_rate = pairs * rows * frame / (band_ms * 1e-3)
        full_rate = pairs * int(wide.len_b[0]) * frame / (full_ms * 1e-3)
        print(json.dumps({"workload": "F", "cpl": cpl, "pairs": pairs, "rows": rows, "band_width": frame,
                          "band_kernel_ms": round(band_ms, 3), "band_frame_cells_per_s": round(band_rate, 0),
                          "score_rows_rows": int(wide.len_b[0]), "score_rows_kernel_ms": round(full_ms, 3),
                          "score_rows_frame_cells_per_s": round(full_rate, 0),
                          "moving_frame_cost": round(full_rate / band_rate, 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="W1,W2,W3,F")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    args = ap.parse_args()
    only = set(args.only.split(","))
    sc = S.make_scoring(SW_SPEC)
    with S.Context(0) as ctx:
        ok = True
        for name in ("W1", "W2", "W3"):
            if name in only:
                ok = run_workload(ctx, sc, name, args) and ok
        if "F" in only:
            run_frame_rate(ctx, sc, args)
    if not ok:
        sys.exit(2)


if __name__ == "__main__":
    main()
