#!/usr/bin/env python3
"""align_banded_wide_bench.py -- the wide banded calls (seqalign_*_banded_wide) against the narrow banded calls and the
unbanded calls, in one process, at every strip width (option band_strip_cols).

Workloads (seeded, edits in equal thirds; NW scoring 1 / -2 / -4 / -1, SW 2 / -3 / -4 / -1):
  W1   1 pair x 100 000 bp, 5 % edits, width <= 1 024 (align_banded_bench.py's B3)   against nw_score_banded / nw_align_banded
  W2   1 000 pairs x 10 000 bp, 8 % edits, w = 256 (B1)                              against nw_score_banded / nw_align_banded
  W3   64 pairs x 20 000 bp, 10 % edits and one 1 500 bp indel, w = 2 048            against nw_score / nw_align_long
  W4   1 000 reads of 10 000 bp in windows of 14 000 bp, 8 % edits, the read's diagonal +- 1 024
                                                                                     against sw_score / sw_batch(max_hits = 1)

One JSON line per workload and strip width: median wall clock of 3 synchronous calls after a warm-up, the wide score call at
every strip width, the wide align call at the widths of --align-cols (default: 0, the library's pick).  Before a line is
printed the tool ASSERTS: W1 / W2 -- the wide results are the narrow calls' for every pair, scores and strings; W3 / W4 --
no wide score is above the unbanded one, the wide align call agrees with the wide score call, and on the first --check
pairs, whose unbanded alignment is computed, the wide result is the unbanded one wherever that walk lies in the band
(in_band counts them).  W3 / W4 carry bar_met: the wide score call took less than the unbanded score call.  --scale divides
the pair counts (a quick run).

    python seq-align_amd/tools/align_banded_wide_bench.py [--only W1,W3] [--cols 0,64,128,256,512] [--scale 1]
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

NW_SPEC = {"init": [1, -2, -4, -1, 0, 0, 0, 0, 0, 0]}
SW_SPEC = {"init": [2, -3, -4, -1, 0, 0, 0, 0, 0, 0]}
ACGT = np.frombuffer(b"ACGT", np.uint8)


def related(rng, n, edits):
    """a random DNA sequence of n and a copy with about `edits` of its positions substituted, deleted or followed by an insertion"""
    a = ACGT[rng.below(4, n).astype(np.int64)]
    kind = rng.below(3000, n).astype(np.int64)
    subs = ACGT[rng.below(4, n).astype(np.int64)]
    cut = int(edits * 1000)
    counts = np.where(kind < cut, 0, np.where(kind < 2 * cut, 2, 1))
    base = np.where((kind >= 2 * cut) & (kind < 3 * cut), subs, a)
    out = np.repeat(base, counts)
    second = (np.cumsum(counts) - 1)[counts == 2]
    out[second] = subs[counts == 2]
    return a.tobytes(), out.tobytes()


def band_of(la, lb, w):
    return max(-lb, min(0, la - lb) - w), min(la, max(0, la - lb) + w)


def excursion(ra, rb, i0=0, j0=0):
    """(lowest, highest) i - j along two gapped strings that start at cell (i0, j0), that cell included"""
    x, y = np.frombuffer(ra, np.uint8) != 0x2D, np.frombuffer(rb, np.uint8) != 0x2D
    d = i0 - j0 + np.cumsum(x.astype(np.int64) - y.astype(np.int64))
    return (min(i0 - j0, int(d.min())), max(i0 - j0, int(d.max()))) if len(d) else (i0 - j0, i0 - j0)


def median_ms(fn, calls, warm):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(t), 2), [round(x, 2) for x in t]


def workload(name, scale):
    """(batch, NW: w per call / SW: (lo, hi) per pair)"""
    if name == "W1":
        rng = W.Rng(1200 + sum(b"B3"))
        a, b = related(rng, 100_000, 0.05)
        return W.from_pairs([(a, b)]), (1024 - abs(len(a) - len(b)) - 1) // 2
    if name == "W2":
        rng = W.Rng(1200 + sum(b"B1"))
        return W.from_pairs([related(rng, 10_000, 0.08) for _ in range(max(1, 1000 // scale))]), 256
    rng = W.Rng(1500 + sum(name.encode()))
    if name == "W3":
        pairs = []
        for k in range(max(1, 64 // scale)):
            a, b = related(rng, 20_000, 0.10)
            at = int(rng.below(len(b) - 3000, 1)[0]) + 1000
            if k % 2:
                b = b[:at] + ACGT[rng.below(4, 1500).astype(np.int64)].tobytes() + b[at:]     # 1 500 bp inserted in seq_b
            else:
                b = b[:at] + b[at + 1500:]                                                     # ... deleted from it
            pairs.append((a, b))
        return W.from_pairs(pairs), 2048
    pairs, lo, hi = [], [], []
    for _ in range(max(1, 1000 // scale)):
        window = ACGT[rng.below(4, 14_000).astype(np.int64)]
        offset = int(rng.below(4001, 1)[0])
        _, read = related_of(rng, window[offset:offset + 10_000], 0.08)
        pairs.append((read, window.tobytes()))
        lo.append(-offset - 1024)
        hi.append(-offset + 1024)
    return W.from_pairs(pairs), (lo, hi)


def related_of(rng, a, edits):
    """related()'s edits applied to a given sequence (uint8 array)"""
    n = len(a)
    kind = rng.below(3000, n).astype(np.int64)
    subs = ACGT[rng.below(4, n).astype(np.int64)]
    cut = int(edits * 1000)
    counts = np.where(kind < cut, 0, np.where(kind < 2 * cut, 2, 1))
    base = np.where((kind >= 2 * cut) & (kind < 3 * cut), subs, a)
    out = np.repeat(base, counts)
    second = (np.cumsum(counts) - 1)[counts == 2]
    out[second] = subs[counts == 2]
    return a.tobytes(), out.tobytes()


def sub_batch(batch, count):
    return W.from_pairs([(batch.seq_a(p), batch.seq_b(p)) for p in range(count)])


def run_nw(ctx, sc, name, args, cols_list, align_cols):
    batch, w = workload(name, args.scale)
    n = batch.n_pairs
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    bands = [band_of(int(a), int(b), w) for a, b in zip(las, lbs)]
    widths = [hi - lo + 1 for lo, hi in bands]
    band_cells = int(sum((int(b) + 1) * wd for b, wd in zip(lbs, widths)))
    head = {"workload": name, "pairs": n, "w": w, "max_width": max(widths), "cells": int((las * lbs).sum()), "band_cells": band_cells}
    narrow = name in ("W1", "W2")
    base_score_fn = (lambda: ctx.nw_score_banded(batch, sc, w)) if narrow else (lambda: ctx.nw_score(batch, sc))
    base_ms, base_all = median_ms(base_score_fn, args.calls, args.warm)
    base_score = base_score_fn()
    head.update(score_base="nw_score_banded" if narrow else "nw_score", score_base_ms=base_ms, score_base_all=base_all)
    n_check = n if narrow else min(n, args.check)
    check = batch if n_check == n else sub_batch(batch, n_check)
    align_fn = (lambda: ctx.nw_align_banded(check, sc, w)) if narrow else (lambda: ctx.nw_align_long(check, sc))
    if narrow:
        a_ms, a_all = median_ms(align_fn, args.calls, args.warm)
        head.update(align_base="nw_align_banded", align_base_ms=a_ms, align_base_all=a_all)
    else:
        t0 = time.perf_counter()
        align_fn()
        head.update(align_base="nw_align_long", align_base_pairs=n_check, align_base_ms=round((time.perf_counter() - t0) * 1e3, 2))
    want = align_fn()
    inside = [True] * n_check
    if not narrow:
        for p in range(n_check):
            lo, hi = excursion(want[p][1], want[p][2])
            inside[p] = bands[p][0] <= lo and hi <= bands[p][1]
    ok = True
    for cols in cols_list:
        out = dict(head, band_strip_cols=cols)
        with ctx.options(band_strip_cols=cols):
            ms, all_ = median_ms(lambda: ctx.nw_score_banded_wide(batch, sc, w), args.calls, args.warm)
            score = ctx.nw_score_banded_wide(batch, sc, w)
            out.update(score_wide_ms=ms, score_wide_all=all_, score_launches=ctx.last_call(), score_speedup=round(base_ms / ms, 2))
            if narrow:
                assert score.tobytes() == base_score.tobytes(), (name, cols, "the wide scores differ from the narrow call's")
            else:
                assert (score <= base_score).all(), (name, cols, "a wide banded score above the unbanded one")
            got = ctx.nw_align_banded_wide(check, sc, w)
            assert [g[0] for g in got] == [int(s) for s in score[:n_check]], (name, cols, "the wide score call disagrees with the wide align call")
            wrong = [p for p in range(n_check) if inside[p] and got[p] != want[p]]
            assert not wrong, (name, cols, "wide result differs from the comparison call's although its path lies in the band", wrong[:5])
            out.update(checked_pairs=n_check, in_band=int(sum(inside)), identical=True)
            if cols in align_cols:
                ms_a, all_a = median_ms(lambda: ctx.nw_align_banded_wide(batch, sc, w), args.calls, args.warm)
                out.update(align_wide_ms=ms_a, align_wide_all=all_a, align_launches=ctx.last_call())
        if not narrow:
            out["bar_met"] = ms < base_ms
            ok = ok and (out["bar_met"] or cols != 0)
        print(json.dumps(out), flush=True)
    return ok


def run_sw(ctx, sc, name, args, cols_list, align_cols):
    batch, (lo, hi) = workload(name, args.scale)
    n = batch.n_pairs
    las, lbs = batch.len_a.astype(np.int64), batch.len_b.astype(np.int64)
    head = {"workload": name, "pairs": n, "half_band": 1024, "max_width": 2049, "cells": int((las * lbs).sum()),
            "band_cells": int(sum(min(int(b), int(a) - max(l, -int(b))) * (min(h, int(a)) - max(l, -int(b)) + 1)
                                  for a, b, l, h in zip(las, lbs, lo, hi)))}
    base_ms, base_all = median_ms(lambda: ctx.sw_score(batch, sc), args.calls, args.warm)
    base = ctx.sw_score(batch, sc)
    head.update(score_base="sw_score", score_base_ms=base_ms, score_base_all=base_all)
    n_check = min(n, args.check)
    check = sub_batch(batch, n_check)
    t0 = time.perf_counter()
    want = ctx.sw_batch(check, sc, 1, max_hits=1)
    head.update(align_base="sw_batch", align_base_pairs=n_check, align_base_ms=round((time.perf_counter() - t0) * 1e3, 2))
    inside = []
    for p in range(n_check):
        if not want[p]:
            inside.append(True)
            continue
        h = want[p][0]
        d_lo, d_hi = excursion(h["a"].encode(), h["b"].encode(), h["pos_a"], h["pos_b"])
        inside.append(lo[p] <= d_lo and d_hi <= hi[p])
    ok = True
    for cols in cols_list:
        out = dict(head, band_strip_cols=cols)
        with ctx.options(band_strip_cols=cols):
            ms, all_ = median_ms(lambda: ctx.sw_score_banded_wide(batch, sc, lo, hi), args.calls, args.warm)
            score, end_a, end_b = ctx.sw_score_banded_wide(batch, sc, lo, hi)
            out.update(score_wide_ms=ms, score_wide_all=all_, score_launches=ctx.last_call(), score_speedup=round(base_ms / ms, 2))
            assert (score <= base[0]).all(), (name, cols, "a wide banded score above the unbanded one")
            got = ctx.sw_align_banded_wide(check, sc, lo[:n_check], hi[:n_check], 1)
            for p in range(n_check):
                g = got[p][0] if got[p] else None
                assert (g["score"] if g else 0) == int(score[p]), (name, cols, p, "the wide score call disagrees with the wide align call")
                if g:
                    assert (g["pos_a"] + g["len_a"], g["pos_b"] + g["len_b"]) == (int(end_a[p]), int(end_b[p])), (name, cols, p)
                if inside[p]:
                    assert got[p] == want[p], (name, cols, p, "wide hit differs from sw_batch's although its walk lies in the band")
            out.update(checked_pairs=n_check, in_band=int(sum(inside)), identical=True)
            if cols in align_cols:
                ms_a, all_a = median_ms(lambda: ctx.sw_align_banded_wide(batch, sc, lo, hi, 1, raw=True), args.calls, args.warm)
                out.update(align_wide_ms=ms_a, align_wide_all=all_a, align_launches=ctx.last_call())
        out["bar_met"] = ms < base_ms
        ok = ok and (out["bar_met"] or cols != 0)
        print(json.dumps(out), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="W1,W2,W3,W4")
    ap.add_argument("--cols", default="0,64,128,256,512")
    ap.add_argument("--align-cols", default="0")
    ap.add_argument("--check", type=int, default=8, help="W3 / W4: pairs whose unbanded alignment is computed for the comparison")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    args = ap.parse_args()
    only = set(args.only.split(","))
    cols_list = [int(c) for c in args.cols.split(",")]
    align_cols = {int(c) for c in args.align_cols.split(",") if c}
    ok = True
    with S.Context(0) as ctx:
        for name in ("W1", "W2", "W3"):
            if name in only:
                ok = run_nw(ctx, S.make_scoring(NW_SPEC), name, args, cols_list, align_cols) and ok
        if "W4" in only:
            ok = run_sw(ctx, S.make_scoring(SW_SPEC), "W4", args, cols_list, align_cols) and ok
    if not ok:
        print("BAR MISSED at the default strip width (see the lines with bar_met false)", file=sys.stderr, flush=True)
        sys.exit(2)


if __name__ == "__main__":
    main()
