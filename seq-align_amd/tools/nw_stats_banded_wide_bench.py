#!/usr/bin/env python3
"""nw_stats_banded_wide_bench.py -- the wide banded NW statistics call (seqalign_nw_stats_banded_wide) next to the routes it
replaces, on the same batch, in one process, at every strip width (option band_strip_cols).

Workloads (seeded, scoring 1 / -2 / -4 / -1, edits in equal thirds):
  A   64 pairs x 20 000 bp, 10 % edits and one 1 500 bp indel, w = 2 048 (align_banded_wide_bench.py's W3)
        against nw_align_banded_wide plus a host count of its strings, and the unbanded nw_stats; nw_score_banded_wide for the ratio
  B   1 pair x 100 000 bp, 5 % edits, w = 255 (511 diagonals: seq_b cut or lengthened to len_a)    against nw_stats_banded (one wave)
  C   1 000 pairs x 10 000 bp, 8 % edits, w = 255 (nw_stats_banded_bench.py's b)                   against nw_stats_banded

One JSON line per workload and strip width.  *_ms: {"median", "min", "max"} of --calls synchronous calls after a warm-up (wall
clock: host arrays in, host arrays out).  The comparison calls are timed once per workload, before the strip widths.
Before a line is printed the tool ASSERTS: the wide scores are nw_score_banded_wide's bit for bit; A -- all three outputs equal
nw_align_banded_wide's score and its counted strings for every pair, and no score is above the unbanded one; B / C -- all three
arrays are nw_stats_banded's byte for byte.  It exits non-zero otherwise.
Aims (set before anything ran; the margin over several processes is the reader's, profiles/r26), in the line of strip width 0:
  A   aim_met: the wide statistics call's median is below align + count's and below the unbanded call's
  B   aim_met: ... below the narrow call's
  C   none: the narrow call is expected to win (one wave per pair is enough where there are a thousand pairs)

    python seq-align_amd/tools/nw_stats_banded_wide_bench.py [--only A,B,C] [--cols 0,64,128,256,512] [--calls 10] [--scale 1]
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
import nw_stats_banded_bench as NB                                        # noqa: E402
from nw_stats_bench import count_columns, timed                           # noqa: E402


def workload(name, scale):
    """(batch, w)"""
    if name == "A":
        return WB.workload("W3", scale)
    if name == "B":
        rng = W.Rng(2600 + sum(b"B"))
        a, b = WB.related(rng, 100_000, 0.05)
        return W.from_pairs([(a, (b + WB.related(rng, 5000, 0.0)[0])[:len(a)])]), 255
    batch, w, _, _ = NB.workload("b", scale)
    return batch, w


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def run_workload(ctx, sc, name, args, cols_list):
    batch, w = workload(name, args.scale)
    n = batch.n_pairs
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    widths = [hi - lo + 1 for lo, hi in (WB.band_of(int(a), int(b), w) for a, b in zip(las, lbs))]
    head = {"workload": name, "pairs": n, "w": w, "min_width": min(widths), "max_width": max(widths), "cells": int((las * lbs).sum()),
            "band_cells": int(sum((int(b) + 1) * wd for b, wd in zip(lbs, widths))), "timed_calls": args.calls}

    def align_and_count():
        return [(score,) + count_columns(sc, ra, rb) for score, ra, rb in ctx.nw_align_banded_wide(batch, sc, w)]

    if name == "A":
        want = align_and_count()
        unbanded = ctx.nw_stats(batch, sc)
        head["align_count_ms"] = timed(align_and_count, args.calls)
        head["stats_unbanded_ms"] = timed(lambda: ctx.nw_stats(batch, sc), args.calls)
        others = [head["align_count_ms"]["median"], head["stats_unbanded_ms"]["median"]]
    else:
        narrow = ctx.nw_stats_banded(batch, sc, w)
        head["stats_narrow_ms"] = timed(lambda: ctx.nw_stats_banded(batch, sc, w), args.calls)
        others = [head["stats_narrow_ms"]["median"]]
    outs = []
    for cols in cols_list:
        out = dict(head, band_strip_cols=cols)
        with ctx.options(band_strip_cols=cols):
            got = ctx.nw_stats_banded_wide(batch, sc, w)
            out["launches"] = ctx.last_call()
            score = ctx.nw_score_banded_wide(batch, sc, w)
            assert got[0].tobytes() == score.tobytes(), (name, cols, "the scores differ from nw_score_banded_wide's")
            if name == "A":
                wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
                assert not wrong, (name, cols, "the wide statistics differ from the wide align call's score and its counted strings", wrong[:5])
                assert (got[0] <= unbanded[0]).all(), (name, cols, "a banded score above the unbanded one")
                out["equals_unbanded"] = int(sum(same_bytes([x[p:p + 1] for x in got], [x[p:p + 1] for x in unbanded]) for p in range(n)))
            else:
                assert same_bytes(got, narrow), (name, cols, "the wide statistics differ from the narrow call's")
            m, mm = got[1].astype(np.int64), got[2].astype(np.int64)
            out["identity_mean"] = round(float(np.mean(m / np.maximum(1, las + lbs - m - mm))), 4)
            out["stats_wide_ms"] = timed(lambda: ctx.nw_stats_banded_wide(batch, sc, w), args.calls)
            out["score_wide_ms"] = timed(lambda: ctx.nw_score_banded_wide(batch, sc, w), args.calls)
        out["stats_over_score_wide"] = round(out["stats_wide_ms"]["median"] / out["score_wide_ms"]["median"], 2)
        out["others_over_stats_wide"] = [round(x / out["stats_wide_ms"]["median"], 2) for x in others]
        out["identical"] = True
        if name != "C":
            out["aim_met"] = bool(out["stats_wide_ms"]["median"] < min(others))
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
    sc = S.make_scoring(WB.NW_SPEC)
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
