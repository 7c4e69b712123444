#!/usr/bin/env python3
"""sw_span_bench.py -- the SW hit-span call (seqalign_sw_span_batch) next to the score-only call and the alignment call it
replaces, on the same batches, in one process.

One JSON line per workload:
  span_kernel_ms   median of >= 20 launches of the span kernels between HIP events (seqalign_sw_span_time_ms), after warm-up
  score_kernel_ms  the same for sw_score's kernels (seqalign_score_time_ms); span_over_score = their ratio
  span_call_ms     median wall clock of >= 10 whole calls: host arrays in, five arrays out
  score_call_ms    the same for seqalign_sw_score_batch
  align_call_ms    the same for seqalign_sw_batch(min_score = 1, max_hits = 1), or for seqalign_sw_align_long where a pair has
                   >= 2^31 cells and sw_batch refuses it (align_call names which)
  launches         what the span call launched (seqalign_ctx_last_call_info)

    python seq-align_amd/tools/sw_span_bench.py [--only C3,C4] [--repeats 20] [--calls 10]
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
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "tests")]

import seqalign_amd as S                      # noqa: E402
from seqalign_amd import workloads as W       # noqa: E402

DNA_SW = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}


def random_pairs(n, la, lb, seed, alphabet=b"ACGT"):
    rng = W.Rng(seed)
    alpha = np.frombuffer(alphabet, np.uint8)
    pairs = []
    for _ in range(n):
        a = alpha[rng.below(len(alpha), la).astype(np.int64)].tobytes()
        b = alpha[rng.below(len(alpha), lb).astype(np.int64)].tobytes()
        pairs.append((a, b))
    return W.from_pairs(pairs)


def workloads():
    yield "C3", lambda: W.dna_sw_read_vs_ref(10000, seed=2), DNA_SW
    yield "C4", lambda: W.protein_sw_300(4000, seed=3), {"preset": "BLOSUM62"}
    yield "reads_700_in_1000", lambda: W.dna_sw_read_vs_ref(10000, seed=4, read_len=700, ref_len=1000), DNA_SW
    yield "sw_5000x5000x64", lambda: random_pairs(64, 5000, 5000, seed=5), DNA_SW
    yield "sw_60000x60000", lambda: random_pairs(1, 60000, 60000, seed=6), DNA_SW


def median_ms(fn, calls, warm_s=0.2):
    t_end = time.perf_counter() + warm_s
    fn()
    while time.perf_counter() < t_end:
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--no-align", action="store_true", help="skip the alignment call (a counter run wants the span kernel alone)")
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    with S.Context(0) as ctx:
        for name, make, spec in workloads():
            if only and name not in only:
                continue
            batch = make()
            sc = S.make_scoring(spec)
            cells = batch.cells()
            repeats = args.repeats
            ctx.sw_span_time_ms(batch, sc, 2)                            # warm-up
            span_ms = ctx.sw_span_time_ms(batch, sc, repeats)
            ctx.score_time_ms(batch, sc, 1, 2)
            score_ms = ctx.score_time_ms(batch, sc, 1, repeats)
            calls, warm = args.calls, (0.0 if cells > 5e8 else 0.2)
            span_call = median_ms(lambda: ctx.sw_span(batch, sc), calls, warm)
            launches = ctx.last_call()
            score_call = median_ms(lambda: ctx.sw_score(batch, sc), calls, warm)
            too_large = bool(((batch.len_a.astype(np.int64) + 1) * (batch.len_b.astype(np.int64) + 1) >= 2 ** 31).any())
            align_ms = None
            if not args.no_align:
                if too_large:
                    align_ms = median_ms(lambda: ctx.sw_align_long(batch, sc, 1), 1, 0.0)
                else:
                    slow = cells > 5e8
                    align_ms = median_ms(lambda: ctx.sw_batch(batch, sc, 1, max_hits=1, raw=True), 3 if slow else args.calls,
                                         0.0 if slow else 0.2)
            k_span, k_score = float(np.median(span_ms)), float(np.median(score_ms))
            print(json.dumps({
                "workload": name, "pairs": batch.n_pairs, "cells": cells, "timed_launches": int(repeats), "timed_calls": int(calls),
                "span_kernel_ms": round(k_span, 4), "score_kernel_ms": round(k_score, 4),
                "span_over_score": round(k_span / k_score, 3), "span_gcups": round(cells / (k_span * 1e-3) / 1e9, 1),
                "span_call_ms": round(span_call, 4), "score_call_ms": round(score_call, 4),
                "align_call": "sw_align_long" if too_large else "sw_batch(max_hits=1)",
                "align_call_ms": None if align_ms is None else round(align_ms, 4),
                "launches": {k: v[0] for k, v in launches.items()}}), flush=True)


if __name__ == "__main__":
    main()
