#!/usr/bin/env python3
"""sw_stats_banded_wide_bench.py -- the wide banded SW statistics call (seqalign_sw_stats_banded_wide) next to the routes it
replaces, on the same batch, in one process, at every strip width (option band_strip_cols).

Workloads (seeded, scoring 2 / -3 / -4 / -1, edits in equal thirds):
  A   1 000 reads of 10 kb with 8 % edits in 14 kb windows, +-1 024 (2 049 diagonals: align_banded_wide_bench.py's W4)
        against sw_align_banded_wide(min_score = 1) plus a host count of its strings, and the unbanded sw_stats;
        sw_score_banded_wide for the ratio
  B   1 000 reads of 10 kb with 8 % edits in 12 kb windows, +-255 (511 diagonals: sw_stats_banded_bench.py's b)
        against sw_stats_banded
  C   1 pair of 60 000 x 60 000 bp, 5 % edits, -255 .. 255 (511 diagonals)      against sw_stats_banded (one wave)

One JSON line per workload and strip width.  *_ms: {"median", "min", "max"} of --calls synchronous calls after a warm-up (wall
clock: host arrays in, host arrays out).  The comparison calls are timed once per workload, before the strip widths.
Before a line is printed the tool ASSERTS: score and pos + len are sw_score_banded_wide's bit for bit; A -- all seven outputs equal
the wide align call's hit and its counted strings for every pair; B / C -- all seven arrays are sw_stats_banded's byte for byte.
It exits non-zero otherwise.
Aims (set before anything ran; the margin over several processes is the reader's, profiles/r27), in the line of strip width 0:
  A   aim_met: the wide statistics call's median is below align + count's and below the unbanded call's
  B   none: the narrow call is expected to win (one wave per pair is enough where there are a thousand pairs)
  C   aim_met: not slower than the narrow call

    python seq-align_amd/tools/sw_stats_banded_wide_bench.py [--only A,B,C] [--cols 0,64,128,256,512] [--calls 10] [--scale 1]
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
from seqalign_amd import workloads as W                                   # noqa: E402
import align_banded_wide_bench as WB                                      # noqa: E402
from sw_span_banded_bench import band_cells, bounds                       # noqa: E402
from sw_stats_bench import hit_fields, timed                              # noqa: E402


def workload(name, scale):
    """(batch, lo, hi)"""
    if name == "A":
        batch, (lo, hi) = WB.workload("W4", scale)
        return batch, np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    if name == "B":
        return bounds("b", scale)
    rng = W.Rng(2700 + sum(b"C"))
    a, b = WB.related(rng, 60_000, 0.05)
    return W.from_pairs([(a, (b + WB.related(rng, 5000, 0.0)[0])[:len(a)])]), np.asarray([-255], np.int32), np.asarray([255], np.int32)


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def run_workload(ctx, sc, name, args, cols_list):
    batch, lo, hi = workload(name, args.scale)
    n = batch.n_pairs
    cells, max_width = band_cells(batch, lo, hi)
    head = {"workload": name, "pairs": n, "max_width": max_width, "cells": batch.cells(), "band_cells": cells, "timed_calls": args.calls}

    def align_and_count():
        return [hit_fields(sc, h) for h in ctx.sw_align_banded_wide(batch, sc, lo, hi, 1)]

    if name == "A":
        want = align_and_count()
        head["align_count_ms"] = timed(align_and_count, args.calls)
        head["stats_unbanded_ms"] = timed(lambda: ctx.sw_stats(batch, sc), args.calls)
        others = [head["align_count_ms"]["median"], head["stats_unbanded_ms"]["median"]]
    else:
        narrow = ctx.sw_stats_banded(batch, sc, lo, hi)
        head["stats_narrow_ms"] = timed(lambda: ctx.sw_stats_banded(batch, sc, lo, hi), args.calls)
        others = [head["stats_narrow_ms"]["median"]]
    outs = []
    for cols in cols_list:
        out = dict(head, band_strip_cols=cols)
        with ctx.options(band_strip_cols=cols):
            got = ctx.sw_stats_banded_wide(batch, sc, lo, hi)
            out["launches"] = ctx.last_call()
            score, end_a, end_b = ctx.sw_score_banded_wide(batch, sc, lo, hi)
            assert np.array_equal(score, got[0]) and np.array_equal(end_a, got[1] + got[3]) and np.array_equal(end_b, got[2] + got[4]), \
                (name, cols, "the statistics call disagrees with sw_score_banded_wide")
            if name == "A":
                wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
                assert not wrong, (name, cols, "the wide statistics differ from the wide align call's hit and its counted strings", wrong[:5])
            else:
                assert same_bytes(got, narrow), (name, cols, "the wide statistics differ from the narrow call's")
            m, mm = got[5].astype(np.int64), got[6].astype(np.int64)
            length = got[3].astype(np.int64) + got[4] - m - mm
            out["hits"] = int((got[0] > 0).sum())
            out["identity_mean"] = round(float(np.mean(m / np.maximum(1, length))), 4)
            out["stats_wide_ms"] = timed(lambda: ctx.sw_stats_banded_wide(batch, sc, lo, hi), args.calls)
            out["score_wide_ms"] = timed(lambda: ctx.sw_score_banded_wide(batch, sc, lo, hi), args.calls)
        out["stats_over_score_wide"] = round(out["stats_wide_ms"]["median"] / out["score_wide_ms"]["median"], 2)
        out["others_over_stats_wide"] = [round(x / out["stats_wide_ms"]["median"], 2) for x in others]
        out["identical"] = True
        if name == "A":
            out["aim_met"] = bool(out["stats_wide_ms"]["median"] < min(others))
        if name == "C":
            out["aim_met"] = bool(out["stats_wide_ms"]["median"] <= min(others))
        print(json.dumps(out), flush=True)
        outs.append(out)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="A,B,C")
    ap.add_argument("--cols", default="0,64,128,256,512")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divides the pair counts (a quick run)")
    args = ap.parse_args()
    cols_list = [int(c) for c in args.cols.split(",")]
    sc = S.make_scoring(WB.SW_SPEC)
    outs = []
    with S.Context(0) as ctx:
        for name in args.only.split(","):
            if name:
                outs += run_workload(ctx, sc, name, args, cols_list)
    for out in outs:
        if out["band_strip_cols"] == 0 and out.get("aim_met") is False:
            print(f"workload {out['workload']}: AIM MISSED at the default strip width", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
