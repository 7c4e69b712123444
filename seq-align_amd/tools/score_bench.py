#!/usr/bin/env python3
"""score_bench.py -- the score-only calls (seqalign_nw_score_batch / seqalign_sw_score_batch) on the BASELINE shapes and on
long pairs, next to the alignment calls on the same batches, in one process.

One JSON line per workload:
  kernel_ms      median of >= 10 launches of the score kernels between HIP events (seqalign_score_time_ms), after warm-up
  gcups          len_a x len_b cells of the batch / kernel_ms
  call_ms        median wall clock of the whole call: host arrays in, scores out
  align_call_ms  the same for seqalign_nw_batch / seqalign_sw_batch(min_score = 1, max_hits = 1) on the same batch
                 (null where that call refuses the batch: pairs of >= 2^31 cells)
  launches       what the score call launched (seqalign_ctx_last_call_info)

    python seq-align_amd/tools/score_bench.py [--only C2,C3] [--repeats 12] [--calls 7]
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
    nw = {"preset": "default"}
    sw = {"init": [2, -2, -2, -1, 0, 0, 0, 0, 0, 0]}
    yield "C2", lambda: W.dna_nw_150(10000, seed=1), nw, 0
    yield "C3", lambda: W.dna_sw_read_vs_ref(10000, seed=2), sw, 1
    yield "C4", lambda: W.protein_sw_300(4000, seed=3), {"preset": "BLOSUM62"}, 1
    yield "nw_5000x5000x64", lambda: random_pairs(64, 5000, 5000, seed=5), nw, 0
    yield "nw_100000x100000", lambda: random_pairs(1, 100000, 100000, seed=6), nw, 0


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
    ap.add_argument("--repeats", type=int, default=12)
    ap.add_argument("--calls", type=int, default=7)
    args = ap.parse_args()
    only = set(filter(None, args.only.split(",")))
    with S.Context(0) as ctx:
        for name, make, spec, is_sw in workloads():
            if only and name not in only:
                continue
            batch = make()
            sc = S.make_scoring(spec)
            cells = batch.cells()
            ctx.score_time_ms(batch, sc, is_sw, 3)                       # warm-up
            ms = ctx.score_time_ms(batch, sc, is_sw, args.repeats)
            kernel_ms = float(np.median(ms))
            score = (lambda: ctx.sw_score(batch, sc)) if is_sw else (lambda: ctx.nw_score(batch, sc))
            long_call = cells > 2e9
            call_ms = median_ms(score, 3 if long_call else args.calls, 0.0 if long_call else 0.2)
            launches = ctx.last_call()
            align_ms = None
            too_large = bool(((batch.len_a.astype(np.int64) + 1) * (batch.len_b.astype(np.int64) + 1) >= 2 ** 31).any())
            if not too_large:
                if is_sw:
                    align = lambda: ctx.sw_batch(batch, sc, 1, max_hits=1, raw=True)   # noqa: E731
                else:
                    align = lambda: ctx.nw_batch(batch, sc, raw=True)                   # noqa: E731
                align_ms = median_ms(align, 3 if cells > 5e8 else args.calls, 0.0 if cells > 5e8 else 0.2)
            print(json.dumps({
                "workload": name, "pairs": batch.n_pairs, "cells": cells, "mode": "sw" if is_sw else "nw",
                "kernel_ms": round(kernel_ms, 4), "kernel_ms_min": round(float(ms.min()), 4),
                "gcups": round(cells / (kernel_ms * 1e-3) / 1e9, 1), "call_ms": round(call_ms, 4),
                "align_call": ("sw_batch(max_hits=1)" if is_sw else "nw_batch") if not too_large else "refused (>= 2^31 cells)",
                "align_call_ms": None if align_ms is None else round(align_ms, 4),
                "launches": {k: v[0] for k, v in launches.items()}}), flush=True)


if __name__ == "__main__":
    main()
