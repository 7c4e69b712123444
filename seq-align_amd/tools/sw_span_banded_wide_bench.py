#!/usr/bin/env python3
"""sw_span_banded_wide_bench.py -- the wide banded SW hit-span call (seqalign_sw_span_banded_wide) next to the other routes to
the five integers of a hit, on the same batch, in one process, at every strip width (option band_strip_cols).

Workloads (seeded, scoring 2 / -3 / -4 / -1, edits in equal thirds):
  A   1 000 reads of 10 kb with 8 % edits in 14 kb windows, +-1 024 (2 049 diagonals: align_banded_wide_bench.py's W4)
        against sw_align_banded_wide(min_score = 1), the unbanded sw_span and sw_stats_banded_wide;
        sw_score_banded_wide for the ratio
  B   16 reads of 200 kb with 5 % edits in 210 kb windows, +-2 048 (4 097 diagonals): past sw_stats_banded_wide's 65 535 letters
        against the unbanded sw_span; sw_score_banded_wide for the ratio
  C   1 000 reads of 10 kb with 8 % edits in 12 kb windows, +-255 (511 diagonals: sw_span_banded_bench.py's b)
        against sw_span_banded

One JSON line per workload and strip width.  *_ms: {"median", "min", "max"} of --calls synchronous calls after a warm-up (wall
clock: host arrays in, host arrays out).  The comparison calls are timed once per workload, before the strip widths.
Before a line is printed the tool ASSERTS: score and pos + len are sw_score_banded_wide's bit for bit; A -- the five outputs equal
the wide align call's hit for every pair and sw_stats_banded_wide's first five byte for byte; B -- sw_stats_banded_wide refuses
the batch (SEQALIGN_E_TOO_LARGE); C -- all five arrays are sw_span_banded's byte for byte.  It exits non-zero otherwise.
Aims (set before anything ran; the margin over several processes is the reader's, profiles/r28), in the line of strip width 0:
  A   aim_met: the wide span call's median is below the align call's and the unbanded span call's, and not above
      sw_stats_banded_wide's
  B   aim_met: below the unbanded span call's
  C   none: the narrow call is expected to win (one wave per pair is enough where there are a thousand pairs)

    python seq-align_amd/tools/sw_span_banded_wide_bench.py [--only A,B,C] [--cols 0,64,128,256,512] [--calls 10] [--scale 1]
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
from sw_stats_bench import timed                                          # noqa: E402


def workload(name, scale):
    """(batch, lo, hi)"""
    if name == "A":
        batch, (lo, hi) = WB.workload("W4", scale)
        return batch, np.asarray(lo, np.int32), np.asarray(hi, np.int32)
    if name == "C":
        return bounds("b", scale)
    rng = W.Rng(2800 + sum(b"B"))
    pairs, lo, hi = [], [], []
    for _ in range(max(1, 16 // scale)):
        window = WB.ACGT[rng.below(4, 210_000).astype(np.int64)]
        offset = int(rng.below(10_001, 1)[0])
        _, read = WB.related_of(rng, window[offset:offset + 200_000], 0.05)
        pairs.append((read, window.tobytes()))
        lo.append(-offset - 2048)
        hi.append(-offset + 2048)
    return W.from_pairs(pairs), np.asarray(lo, np.int32), np.asarray(hi, np.int32)


def same_bytes(x, y):
    return len(x) == len(y) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(x, y))


def hit_five(hits):
    h = hits[0] if hits else None
    return (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0)


def run_workload(ctx, sc, name, args, cols_list):
    batch, lo, hi = workload(name, args.scale)
    n = batch.n_pairs
    cells, max_width = band_cells(batch, lo, hi)
    head = {"workload": name, "pairs": n, "max_width": max_width, "cells": batch.cells(), "band_cells": cells, "timed_calls": args.calls}
    want = narrow = stats = None
    lower, not_above = [], []       # medians the wide span call must stay below / must not exceed
    if name == "A":
        want = [hit_five(h) for h in ctx.sw_align_banded_wide(batch, sc, lo, hi, 1)]
        head["align_wide_ms"] = timed(lambda: ctx.sw_align_banded_wide(batch, sc, lo, hi, 1), args.calls)
        stats = ctx.sw_stats_banded_wide(batch, sc, lo, hi)
        head["stats_wide_ms"] = timed(lambda: ctx.sw_stats_banded_wide(batch, sc, lo, hi), args.calls)
        lower.append(head["align_wide_ms"]["median"])
        not_above.append(head["stats_wide_ms"]["median"])
    if name == "B":
        try:
            ctx.sw_stats_banded_wide(batch, sc, lo, hi)
            raise AssertionError("sw_stats_banded_wide accepted sequences of more than 65 535 letters")
        except S.SeqAlignError as e:
            assert e.code == S.E_TOO_LARGE, str(e)
    if name in ("A", "B"):
        unbanded = ctx.sw_span(batch, sc)
        head["span_unbanded_ms"] = timed(lambda: ctx.sw_span(batch, sc), args.calls)
        lower.append(head["span_unbanded_ms"]["median"])
    if name == "C":
        narrow = ctx.sw_span_banded(batch, sc, lo, hi)
        head["span_narrow_ms"] = timed(lambda: ctx.sw_span_banded(batch, sc, lo, hi), args.calls)
    outs = []
    for cols in cols_list:
        out = dict(head, band_strip_cols=cols)
        with ctx.options(band_strip_cols=cols):
            got = ctx.sw_span_banded_wide(batch, sc, lo, hi)
            out["launches"] = ctx.last_call()
            score, end_a, end_b = ctx.sw_score_banded_wide(batch, sc, lo, hi)
            assert np.array_equal(score, got[0]) and np.array_equal(end_a, got[1] + got[3]) and np.array_equal(end_b, got[2] + got[4]), \
                (name, cols, "the span call disagrees with sw_score_banded_wide")
            if name == "A":
                wrong = [p for p in range(n) if tuple(int(x[p]) for x in got) != want[p]]
                assert not wrong, (name, cols, "the wide spans differ from the wide align call's hit", wrong[:5])
                assert same_bytes(got, stats[:5]), (name, cols, "the wide spans differ from sw_stats_banded_wide's first five")
            if name == "C":
                assert same_bytes(got, narrow), (name, cols, "the wide spans differ from the narrow call's")
            if name in ("A", "B"):
                out["equal_to_unbanded"] = int(sum(all(int(x[p]) == int(y[p]) for x, y in zip(got, unbanded)) for p in range(n)))
            out["hits"] = int((got[0] > 0).sum())
            out["pos_a_max"] = int(got[1].max())
            out["span_wide_ms"] = timed(lambda: ctx.sw_span_banded_wide(batch, sc, lo, hi), args.calls)
            out["score_wide_ms"] = timed(lambda: ctx.sw_score_banded_wide(batch, sc, lo, hi), args.calls)
        mine = out["span_wide_ms"]["median"]
        out["span_over_score_wide"] = round(mine / out["score_wide_ms"]["median"], 2)
        for key in ("align_wide_ms", "stats_wide_ms", "span_unbanded_ms", "span_narrow_ms"):
            if key in head:
                out[key[:-3] + "_over_span_wide"] = round(head[key]["median"] / mine, 2)
        out["identical"] = True
        if name in ("A", "B"):
            out["aim_met"] = bool(all(mine < x for x in lower) and all(mine <= x for x in not_above))
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
