#!/usr/bin/env python3
"""sw_span_banded_bench.py -- the banded SW hit-span call (seqalign_sw_span_banded) next to the banded score call, the banded
alignment call it replaces and the unbanded span call, on the same batches, in one process.

Workloads (align_banded_sw_bench.py's batches and planted offsets; the band is the read's true offset in its window +- w):
  a   10 000 reads of 700 bp in 1 000 bp windows, w = 32 (65 diagonals: 2 per lane)
  b   1 000 reads of 10 kb with 8 % edits in 12 kb windows, w = 255 (511 diagonals: 8 per lane; +-256 is over the call's cap)

One JSON line per workload:
  span_banded_kernel_ms    median of >= 20 launches between HIP events (seqalign_sw_span_band_time_ms), after a warm-up
  score_banded_kernel_ms   the same for seqalign_sw_score_banded (seqalign_sw_band_score_time_ms)
  span_banded_call_ms      median wall clock of >= 10 whole calls: host arrays in, five arrays out
  score_banded_call_ms, align_banded_call_ms (raw: no Python dict per hit), span_call_ms (the unbanded seqalign_sw_span_batch)
  aim_met                  the aim set before anything ran: the span-banded call is faster than the align-banded call
Before a line is printed the tool ASSERTS that the span call's five fields are the align call's hit fields for every pair and
that its score and pos + len are the score call's; it exits non-zero otherwise.

    python seq-align_amd/tools/sw_span_banded_bench.py [--only a,b] [--repeats 20] [--calls 10] [--scale 1]
    ... --counter-run     one span-banded and one score-banded call on workload a, nothing else (for a counter pass)
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "seq-align_amd" / "tools")]

import seqalign_amd as S                                   # noqa: E402
from align_banded_sw_bench import SW_SPEC, workload        # noqa: E402
from sw_span_bench import median_ms                        # noqa: E402

WORKLOADS = {"a": ("W1", 32), "b": ("W2", 255)}


def bounds(name, scale):
    batch, start, _ = workload(WORKLOADS[name][0], scale)
    w = WORKLOADS[name][1]
    return batch, (-start - w).astype(np.int32), (-start + w).astype(np.int32)


def band_cells(batch, lo, hi):
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    d_lo, d_hi = np.maximum(lo, -lbs), np.minimum(hi, las)
    rows = np.maximum(0, np.minimum(lbs, las - d_lo) - np.maximum(1, 1 - d_hi) + 1)
    return int((rows * (d_hi - d_lo + 1)).sum()), int((d_hi - d_lo + 1).max())


def run_workload(ctx, sc, name, args):
    batch, lo, hi = bounds(name, args.scale)
    n = batch.n_pairs
    cells, max_width = band_cells(batch, lo, hi)
    # results first: the span call against the align call and the score call
    got = ctx.sw_span_banded(batch, sc, lo, hi)
    launches = ctx.last_call()
    hits = ctx.sw_align_banded(batch, sc, lo, hi, 1)
    want = [(h[0]["score"], h[0]["pos_a"], h[0]["pos_b"], h[0]["len_a"], h[0]["len_b"]) if h else (0, 0, 0, 0, 0) for h in hits]
    wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
    assert not wrong, (name, "the span call differs from the align call's hit", wrong[:5])
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    assert np.array_equal(score, got[0]) and np.array_equal(end_a, got[1] + got[3]) and np.array_equal(end_b, got[2] + got[4]), \
        (name, "the span call disagrees with the score call")
    repeats, calls = args.repeats, args.calls
    ctx.sw_span_band_time_ms(batch, sc, lo, hi, 2)                        # warm-up
    k_span = float(np.median(ctx.sw_span_band_time_ms(batch, sc, lo, hi, repeats)))
    ctx.sw_band_score_time_ms(batch, sc, lo, hi, 2)
    k_score = float(np.median(ctx.sw_band_score_time_ms(batch, sc, lo, hi, repeats)))
    span_call = median_ms(lambda: ctx.sw_span_banded(batch, sc, lo, hi), calls)
    score_call = median_ms(lambda: ctx.sw_score_banded(batch, sc, lo, hi), calls)
    align_call = median_ms(lambda: ctx.sw_align_banded(batch, sc, lo, hi, 1, raw=True), calls)
    full_call = median_ms(lambda: ctx.sw_span(batch, sc), calls, 0.0)
    out = {"workload": name, "pairs": n, "w": WORKLOADS[name][1], "max_width": max_width, "band_cells": cells, "cells": batch.cells(),
           "timed_launches": int(repeats), "timed_calls": int(calls),
           "span_banded_kernel_ms": round(k_span, 4), "score_banded_kernel_ms": round(k_score, 4),
           "span_over_score_kernel": round(k_span / k_score, 3), "span_banded_band_gcups": round(cells / (k_span * 1e-3) / 1e9, 1),
           "span_banded_call_ms": round(span_call, 4), "score_banded_call_ms": round(score_call, 4),
           "align_banded_call_ms": round(align_call, 4), "span_call_ms": round(full_call, 4),
           "hits": int((got[0] > 0).sum()), "equals_align_call": True, "equals_score_call": True,
           "launches": {k: v[0] for k, v in launches.items()}, "aim_met": bool(span_call < align_call)}
    print(json.dumps(out), flush=True)
    return out["aim_met"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the pair counts (a quick run)")
    ap.add_argument("--counter-run", action="store_true", help="one span-banded and one score-banded call on workload a, nothing else")
    args = ap.parse_args()
    sc = S.make_scoring(SW_SPEC)
    with S.Context(0) as ctx:
        if args.counter_run:
            batch, lo, hi = bounds("a", args.scale)
            ctx.sw_span_banded(batch, sc, lo, hi)
            ctx.sw_score_banded(batch, sc, lo, hi)
            print(json.dumps({"workload": "a", "pairs": batch.n_pairs, "band_cells": band_cells(batch, lo, hi)[0]}), flush=True)
            return 0
        met = [run_workload(ctx, sc, name, args) for name in args.only.split(",") if name]
    for name, ok in zip(args.only.split(","), met):
        if not ok:
            print(f"workload {name}: AIM MISSED: the span-banded call is not faster than the align-banded call", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
