#!/usr/bin/env python3
"""sw_stats_banded_bench.py -- the banded SW statistics call (seqalign_sw_stats_banded) next to the banded span and score calls,
the banded alignment call plus a host count of its strings (the route it replaces) and the unbanded statistics call, on the same
batch, in one process.

Workloads (sw_span_banded_bench.py's: the band is the read's true offset in its window +- w):
  a   10 000 reads of 700 bp in 1 000 bp windows, w = 32 (65 diagonals: 2 per lane)
  b   1 000 reads of 10 kb with 8 % edits in 12 kb windows, w = 255 (511 diagonals: 8 per lane)

One JSON line per workload.  *_kernel_ms: {"median", "min", "max"} of --repeats launches between HIP events after a warm-up
(seqalign_sw_stats_band_time_ms, seqalign_sw_span_band_time_ms, seqalign_sw_band_score_time_ms; the batch uploaded once).
*_call_ms: the same of --calls whole calls (wall clock: host arrays in, host arrays out):
  stats_banded_*          seqalign_sw_stats_banded
  span_banded_*           seqalign_sw_span_banded
  score_banded_*          seqalign_sw_score_banded
  align_count_call_ms     seqalign_sw_align_banded(min_score = 1) plus counting the columns of its strings on the host
  stats_call_ms           the unbanded seqalign_sw_stats_batch
Aims, set before anything ran and recorded as met or missed:
  aim_kernel              stats_banded_kernel_ms <= span_banded_kernel_ms (medians of this process; the margin over several
                          processes is the reader's: profiles/r23)
  aim_call_met            stats_banded_call_ms < align_count_call_ms and < stats_call_ms (medians)
Before a line is printed the tool ASSERTS that the first five outputs are seqalign_sw_span_banded's bit for bit, that score and
pos + len are seqalign_sw_score_banded's, and that all seven equal the alignment call's hit and its counted strings for every
pair; it exits non-zero otherwise.

    python seq-align_amd/tools/sw_stats_banded_bench.py [--only a,b] [--repeats 20] [--calls 10] [--scale 1]
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT / "seq-align_amd" / "python"), str(ROOT / "seq-align_amd" / "tools")]

import seqalign_amd as S                                                  # noqa: E402
from align_banded_sw_bench import SW_SPEC                                 # noqa: E402
from sw_span_banded_bench import WORKLOADS, band_cells, bounds            # noqa: E402
from sw_stats_bench import hit_fields, spread, timed                      # noqa: E402


def run_workload(ctx, sc, name, args):
    batch, lo, hi = bounds(name, args.scale)
    n = batch.n_pairs
    cells, max_width = band_cells(batch, lo, hi)

    def align_and_count():
        return [hit_fields(sc, h) for h in ctx.sw_align_banded(batch, sc, lo, hi, 1)]

    # results first: against the span call, the score call and the align call's counted strings
    got = ctx.sw_stats_banded(batch, sc, lo, hi)
    launches = ctx.last_call()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:5], ctx.sw_span_banded(batch, sc, lo, hi))), \
        (name, "the first five outputs differ from sw_span_banded's")
    score, end_a, end_b = ctx.sw_score_banded(batch, sc, lo, hi)
    assert np.array_equal(score, got[0]) and np.array_equal(end_a, got[1] + got[3]) and np.array_equal(end_b, got[2] + got[4]), \
        (name, "the statistics call disagrees with the score call")
    want = align_and_count()
    wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
    assert not wrong, (name, "the statistics call differs from the align call's hit and its counted strings", wrong[:5])
    m, mm = got[5].astype(np.int64), got[6].astype(np.int64)
    length = got[3].astype(np.int64) + got[4] - m - mm

    repeats, calls = args.repeats, args.calls
    out = {"workload": name, "pairs": n, "w": WORKLOADS[name][1], "max_width": max_width, "band_cells": cells, "cells": batch.cells(),
           "timed_launches": int(repeats), "timed_calls": int(calls), "hits": int((got[0] > 0).sum()),
           "identity_mean": round(float(np.mean(m / np.maximum(1, length))), 4)}
    ctx.sw_stats_band_time_ms(batch, sc, lo, hi, 2)                       # warm-up
    out["stats_banded_kernel_ms"] = spread(ctx.sw_stats_band_time_ms(batch, sc, lo, hi, repeats))
    ctx.sw_span_band_time_ms(batch, sc, lo, hi, 2)
    out["span_banded_kernel_ms"] = spread(ctx.sw_span_band_time_ms(batch, sc, lo, hi, repeats))
    ctx.sw_band_score_time_ms(batch, sc, lo, hi, 2)
    out["score_banded_kernel_ms"] = spread(ctx.sw_band_score_time_ms(batch, sc, lo, hi, repeats))
    out["stats_over_span_kernel"] = round(out["stats_banded_kernel_ms"]["median"] / out["span_banded_kernel_ms"]["median"], 3)
    out["stats_over_score_kernel"] = round(out["stats_banded_kernel_ms"]["median"] / out["score_banded_kernel_ms"]["median"], 3)
    out["stats_banded_band_gcups"] = round(cells / (out["stats_banded_kernel_ms"]["median"] * 1e-3) / 1e9, 1)
    out["stats_banded_call_ms"] = timed(lambda: ctx.sw_stats_banded(batch, sc, lo, hi), calls)
    out["span_banded_call_ms"] = timed(lambda: ctx.sw_span_banded(batch, sc, lo, hi), calls)
    out["score_banded_call_ms"] = timed(lambda: ctx.sw_score_banded(batch, sc, lo, hi), calls)
    out["align_count_call_ms"] = timed(align_and_count, calls)
    out["stats_call_ms"] = timed(lambda: ctx.sw_stats(batch, sc), calls)
    out["align_count_over_stats_banded_call"] = round(out["align_count_call_ms"]["median"] / out["stats_banded_call_ms"]["median"], 2)
    out["stats_over_stats_banded_call"] = round(out["stats_call_ms"]["median"] / out["stats_banded_call_ms"]["median"], 2)
    out["equals_span_call"] = out["equals_score_call"] = out["equals_align_count"] = True
    out["launches"] = {k: v[0] for k, v in launches.items()}
    out["aim_kernel"] = "met" if out["stats_banded_kernel_ms"]["median"] <= out["span_banded_kernel_ms"]["median"] else "missed"
    out["aim_call_met"] = bool(out["stats_banded_call_ms"]["median"] < min(out["align_count_call_ms"]["median"], out["stats_call_ms"]["median"]))
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the pair counts (a quick run)")
    args = ap.parse_args()
    sc = S.make_scoring(SW_SPEC)
    with S.Context(0) as ctx:
        outs = [run_workload(ctx, sc, name, args) for name in args.only.split(",") if name]
    for out in outs:
        if out["aim_kernel"] != "met":
            print(f"workload {out['workload']}: the statistics kernel's median is above the span kernel's in this process", file=sys.stderr, flush=True)
        if not out["aim_call_met"]:
            print(f"workload {out['workload']}: AIM MISSED: the call is not faster than align + count and the unbanded call", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
