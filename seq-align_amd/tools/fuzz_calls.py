#!/usr/bin/env python3
"""Differential fuzz of the score-family calls against the oracle: seqalign_*_score_batch, seqalign_sw_span_batch, *_score_cross,
*_score_search, seqalign_sw_span_cross and seqalign_sw_span_search (against sw_span on the explicit batch), seqalign_nw_stats_batch
(the columns of the oracle's strings) and seqalign_nw_stats_cross (against nw_stats on the explicit batch), seqalign_sw_stats_batch
(the oracle's first hit and its counted strings) and seqalign_sw_stats_cross (against sw_stats on the explicit batch), *_align_long, the banded NW calls,
seqalign_nw_stats_banded (the counted strings of the oracle's walk over the banded matrices; the lowest pair without an alignment inside its
band named), seqalign_sw_span_banded, seqalign_sw_stats_banded (the oracle's
banded hit and its counted strings) and (on from the command line, --no-wide leaves them out) the four wide banded score and align calls,
seqalign_sw_span_banded_wide, seqalign_nw_stats_banded_wide and seqalign_sw_stats_banded_wide (each with its narrow call's bytes on the small pairs),
and seqalign_sw_counts_batch / _banded / _banded_wide (each against the sw_stats and the sw_score call of the same geometry on the same batch),
and seqalign_sw_gaps_batch / _banded / _banded_wide (the '-' runs of the oracle's strings on the same batches; no random draw of their own),
seqalign_nw_gaps_batch / _cross / _banded / _banded_wide (the '-' runs of the oracle's NW strings on the nw_stats calls' batches and bands; no random draw of their own), under random scorings (penalties, the five flags, case sensitivity, a wildcard,
mutations that differ by direction) on random, related and tandem-repeat pairs, some wider than 1 024 columns.

    python seq-align_amd/tools/fuzz_calls.py --seconds 300

tests/test_gpu_soak_calls.py runs seeded slices of it (run(seconds, seed, max_trials)) under the `gpu` marker; the long slices
leave the wide banded calls out (their Python reference on bands past 1 024 diagonals takes most of a second a trial), a
short one runs them.
"""
import argparse
import random
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "seq-align_amd" / "python"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401

import bandlib as BL  # noqa: E402
import bandswlib as BS  # noqa: E402
import orclib as O  # noqa: E402
import statlib as ST  # noqa: E402
import seqalign_amd as S  # noqa: E402
from seqalign_amd import workloads as W  # noqa: E402


def best_cell(M, la, lb):
    """(score, end_a, end_b) of the SW score calls from the oracle's match_scores: score desc, column asc, row asc."""
    Mr = np.asarray(M, np.int64).reshape(lb + 1, la + 1)
    best = int(Mr.max())
    if best <= 0:
        return 0, 0, 0
    rows, cols = np.nonzero(Mr == best)
    k = np.lexsort((rows, cols))[0]
    return best, int(cols[k]), int(rows[k])


def top_k(score, end_a, end_b, k, min_score):
    """The search calls' contract on dense matrices: per query (targets, scores, end_a, end_b), score desc then target asc."""
    out = []
    for row, ea, eb in zip(score, end_a, end_b):
        idx = np.nonzero(row.astype(np.int64) >= min_score)[0]
        order = idx[np.lexsort((idx, -row[idx].astype(np.int64)))][:k]
        out.append((order, row[order], ea[order], eb[order]))
    return out


def walked_along_the_floor(osc, a, b, w, ra, rb):
    """Whether the strings of the oracle's walk over the banded NW matrices are no alignment of the banded problem: they leave
    the band, or under no_mismatches they hold a column of two letters that the scoring does not call a match -- the align
    walker stepping along cells at the floor (include/seqalign_hip.h, banded NW statistics).  seqalign_nw_stats_banded refuses
    such a pair.  (tests/bandnwstatlib.py states the same rule for the tests; the tool keeps its own and takes from the test
    helpers only bandlib's geometry and statlib's lookup.)"""
    if not BL.in_band(ra, rb, len(a), len(b), w):
        return True
    look = ST.Lookup(osc)
    return bool(osc.no_mismatches) and any(x != 45 and y != 45 and not look(x, y)[1] for x, y in zip(ra, rb))


SCALE_LOW_BITS = 8      # the drawn factors start at 2^8


def counts_view(seven):
    """(score, end_a, end_b, matches, mismatches) arrays of a sw_stats call's seven: what the sw_counts call of the same geometry
    must return byte for byte."""
    return [seven[0], seven[1] + seven[3], seven[2] + seven[4], seven[5], seven[6]]


def gaps_want(h):
    """(score, end_a, end_b, gap_runs_a, gap_runs_b) of an oracle hit dict or None: what the sw_gaps call of that geometry returns."""
    if not h:
        return (0, 0, 0, 0, 0)
    runs = tuple(sum(1 for k, ch in enumerate(t) if ch == "-" and (k == 0 or t[k - 1] != "-")) for t in (h["a"], h["b"]))
    return (h["score"], h["pos_a"] + h["len_a"], h["pos_b"] + h["len_b"]) + runs


def dash_runs(s) -> int:
    """Maximal runs of '-' in one string of an alignment (bytes)."""
    return sum(1 for k in range(len(s)) if s[k] == 45 and (k == 0 or s[k - 1] != 45))


def gaps_got(res):
    return [tuple(int(x[k]) for x in res) for k in range(len(res[0]))]


def scaled_spec(spec, f):
    """Every number of the scoring times f: match, mismatch, the gap penalties, wildcard and mutation scores."""
    out = dict(spec, init=[x * f for x in spec["init"][:4]] + list(spec["init"][4:]),
               wildcards=[[c, x * f] for c, x in spec["wildcards"]])
    if "mutations" in spec:
        out["mutations"] = [[x, y, z * f] for x, y, z in spec["mutations"]]
    return out


def draw_factor(G, srng, scale, spec, peak1, la, lb):
    """G: tests/maglib.py (the documented magnitude bound, restated).  (factor, redraws): a factor drawn log-uniformly from
    2^8 .. scale, odd so that the low bits are populated; a draw under
    which the exact-integer peak f * peak1 (peak1: the pairs' largest |value| at factor 1 plus the largest |penalty| -- the
    recurrence is homogeneous) leaves int32, or which the library's documented bound refuses (include/seqalign_hip.h,
    SEQALIGN_E_DOMAIN; maglib.admitted), is drawn again and counted."""
    redraws = 0
    while True:
        u = float(srng.unit(1)[0])
        f = int(2 ** (SCALE_LOW_BITS + u * (np.log2(scale) - SCALE_LOW_BITS))) | 1
        big = scaled_spec(spec, f)
        if f * peak1 <= G.INT32_MAX and all(G.admitted(big, la, lb, call) for call in ("score", "band")):
            return f, redraws
        redraws += 1


def run(seconds=120.0, seed=1, max_trials=1 << 60, ctx=None, wide_calls=False, scale=1, dry=False):
    """Fuzz until `seconds` have passed or `max_trials` scorings were drawn; SystemExit(1) on the first mismatch, with the
    failing case printed.  Options it sets (long_block_rows, band_strip_cols) are put back before it returns or raises.
    wide_calls: also the four *_banded_wide calls, on bands on both sides of 1 024 diagonals and random strip widths.
    scale: above 1, every trial's scoring is multiplied by a factor of up to `scale` (draw_factor; its draws come from a
    generator of their own, and with the default of 1 the drawn stream is what it always was).  dry: draw and count only --
    no device call -- for the CPU check of the redraw share."""
    rng = W.Rng(seed)
    srng = W.Rng(seed ^ 0x5CA1E) if scale != 1 else None
    if srng is not None:
        import maglib as G      # only the scaled runs need it: the default run is what it was, imports included
    ctx = ctx or (None if dry else S.Context(0))
    t_end = time.time() + seconds
    n = {"trials": 0, "redraws": 0, "redrawn_trials": 0, "nw_trials": 0, "score": 0, "cross": 0, "search": 0, "long": 0, "banded": 0, "banded_none": 0, "wide": 0, "banded_wide": 0, "span_banded_wide": 0, "span": 0, "span_banded": 0, "span_cross": 0, "span_search": 0, "stats": 0, "stats_cross": 0, "sw_stats": 0, "sw_stats_cross": 0, "sw_stats_banded": 0,
         "stats_banded": 0, "stats_banded_none": 0, "stats_banded_wide": 0, "sw_stats_banded_wide": 0,
         "sw_counts": 0, "sw_counts_banded": 0, "sw_counts_banded_wide": 0,
         "sw_gaps": 0, "sw_gaps_banded": 0, "sw_gaps_banded_wide": 0,
         "nw_gaps": 0, "nw_gaps_cross": 0, "nw_gaps_banded": 0, "nw_gaps_banded_wide": 0}

    def rand(count, alpha=b"ACGT"):
        return bytes(alpha[i] for i in rng.below(len(alpha), count)) if count else b""

    def fail(what, spec, *details):
        print(f"{what} MISMATCH", spec, *details, flush=True)
        raise SystemExit(1)

    def nw_stats_banded_check(what, call, narrow, spec, sub, bands, both, n_small, count=None):
        """seqalign_nw_stats_banded(_wide) on pairs whose banded (end value, walk) `both` holds: the end value and the counted
        columns of the walk's strings; the pairs the oracle does not walk inside their band (walked_along_the_floor
        included) make the call fail with the lowest of them named, and the rest runs without them.  narrow: the call whose
        bytes `call` must return on the first n_small pairs.  count: what the call counts over the walk's two strings (default:
        the statistics' columns; the gap-run calls: dash_runs of each).  Returns (pairs equal to the oracle, pairs without an
        alignment)."""
        count = count or (lambda ra, rb: ST.count_columns(osc, ra, rb))
        want = [None if x[1] is None or walked_along_the_floor(osc, a, b, w, x[1][1], x[1][2]) else (x[0],) + count(x[1][1], x[1][2])
                for (a, b), w, x in zip(sub, bands, both)]
        none = [k for k, x in enumerate(want) if x is None]
        if none:
            try:
                call(W.from_pairs(sub), sc, bands)
                fail(what + " NONE", spec, sub, bands, none, "no error")
            except S.SeqAlignError as e:
                if e.code != S.E_TRACEBACK or f"pair {none[0]}:" not in str(e):
                    fail(what + " NONE", spec, sub, bands, none, str(e))
        keep = [k for k in range(len(sub)) if k not in none]
        if keep:
            res = call(W.from_pairs([sub[k] for k in keep]), sc, [bands[k] for k in keep])
            got = ST.got_stats(res)
            if got != [want[k] for k in keep]:
                fail(what, spec, [sub[k] for k in keep], [bands[k] for k in keep], got, [want[k] for k in keep])
            small = [k for k in keep if k < n_small]
            if narrow is not None and small:
                wide_res = call(W.from_pairs([sub[k] for k in small]), sc, [bands[k] for k in small])
                narrow_res = narrow(W.from_pairs([sub[k] for k in small]), sc, [bands[k] for k in small])
                if any(x.tobytes() != y.tobytes() for x, y in zip(wide_res, narrow_res)):
                    fail("WIDE / NARROW " + what, spec, [sub[k] for k in small], [bands[k] for k in small])
        return len(keep), len(none)

    while time.time() < t_end and n["trials"] < max_trials:
        v = rng.below(1 << 20, 16).astype(int)
        flags = [int(v[0] >> k) & 1 for k in range(5)]
        if v[15] % 5 < 3:
            flags = [0, 0, 0, 0, 0]
        match, mismatch = int(1 + v[1] % 4), -int(v[2] % 13)     # (0 .. -12: below 2 (gap_open + gap_extend) in a good share of the draws -- insertion runs directly against deletion runs, tests/denselib.py)
        go, ge = -int(v[3] % 8), -int(v[4] % 3)
        if flags[2] and flags[3]:
            mismatch = min(mismatch, go + ge)
        case = int(v[5] & 1)
        spec = {"init": [match, mismatch, go, ge, *flags, case], "wildcards": [["N", int(v[6] % 3) - 1]] if v[6] & 1 else []}
        if n["trials"] % 3 == 2:      # mutations are stored as given (no case folding): in the case the lookup will ask for
            x, y = ("A", "C") if case else ("a", "c")
            spec["mutations"] = [[x, y, -int(1 + v[7] % 3)], [y, x, int(v[8] % 3)]]
        sc = S.make_scoring(spec)
        osc = O.Scoring.from_buffer_copy(bytes(sc))
        nw_ok = min(osc.gap_open + osc.gap_extend, osc.gap_extend) >= -abs(osc.min_penalty)   # NW parity domain

        pairs = []
        wide = int(v[9] % 12) if n["trials"] % 2 else -1     # every second trial: one pair of more than 1 024 columns
        for k in range(12):
            kind = int(v[7] + k) % 3
            la = int(2 + (v[8] * (k + 1)) % (260 if k % 4 else 900))
            if k == wide:
                la = int(1025 + v[10] % 600)
            if kind == 0:
                a, b = rand(la), rand(int(2 + (v[9] * (k + 3)) % 200))
            elif kind == 1:
                a = rand(la)
                cut = int(v[10] % max(1, len(a)))
                b = rand(int(v[11] % 30)) + a[cut:cut + 120] + rand(int(v[12] % 30))
            else:
                unit = rand(int(2 + v[13] % 7))
                a, b = unit * int(2 + v[14] % 20), rand(3) + unit * int(2 + v[15] % 25)
                if k == wide:
                    a = unit * (la // len(unit) + 1)
            if spec["wildcards"] and k % 5 == 0:
                a = a[:len(a) // 2] + b"N" + a[len(a) // 2:]
            if k % 4 == 1:                                    # some lower case: folded, or a mismatch when case_sensitive
                b = b[:len(b) // 3] + b[len(b) // 3:2 * len(b) // 3].lower() + b[2 * len(b) // 3:]
            pairs.append((a, b))
        n["wide"] += sum(len(a) > 1024 for a, _ in pairs)
        batch = W.from_pairs(pairs)
        thr = int(1 + v[5] % (6 * match))

        # ---- the oracle, once per pair and mode
        fills = {}
        for is_sw in ((0, 1) if nw_ok else (1,)):
            for p, (a, b) in enumerate(pairs):
                rc, M, A, B = O.oracle_fill(osc, a, b, is_sw)
                if rc != 0:
                    fail("ORACLE", spec, p, pairs[p])
                fills[is_sw, p] = (M, A, B)

        if srng is not None:     # the same pairs under the scoring times a drawn factor
            peak1 = max(G.cells_peak(*f3) for f3 in fills.values()) + max(abs(x) for x in G.numbers(spec) + [w[1] for w in spec["wildcards"]])
            factor, redraws = draw_factor(G, srng, scale, spec, peak1, max(len(a) for a, _ in pairs), max(len(b) for _, b in pairs))
            n["redraws"] += redraws
            n["redrawn_trials"] += redraws > 0
            spec = scaled_spec(spec, factor)
            sc = S.make_scoring(spec)
            osc = O.Scoring.from_buffer_copy(bytes(sc))
            thr *= factor
            if not dry:
                for (is_sw, p) in list(fills):
                    rc, M, A, B = O.oracle_fill(osc, *pairs[p], is_sw)
                    if rc != 0:
                        fail("ORACLE", spec, p, pairs[p])
                    fills[is_sw, p] = (M, A, B)
        if dry:
            n["trials"] += 1
            n["nw_trials"] += nw_ok
            continue

        # ---- score only
        if nw_ok:
            got = ctx.nw_score(batch, sc)
            for p in range(12):
                M, A, B = fills[0, p]
                if int(got[p]) != int(max(M[-1], A[-1], B[-1])):
                    fail("NW SCORE", spec, p, pairs[p], int(got[p]))
        s, ea, eb = ctx.sw_score(batch, sc)
        for p, (a, b) in enumerate(pairs):
            want = best_cell(fills[1, p][0], len(a), len(b))
            if (int(s[p]), int(ea[p]), int(eb[p])) != want:
                fail("SW SCORE", spec, p, pairs[p], (int(s[p]), int(ea[p]), int(eb[p])), want)
        n["score"] += 12 * (1 + nw_ok)

        # ---- SW hit spans: the oracle's first hit without its strings; SW statistics: that hit and its strings' counted columns
        got = ctx.sw_span(batch, sc)
        got7 = ctx.sw_stats(batch, sc)
        want_runs = []
        for p, (a, b) in enumerate(pairs):
            rc, hits = O.oracle_sw_hits(osc, a, b, *fills[1, p], 1, 1)
            h = hits[0] if hits else None
            want = (h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0)
            if rc != 0 or tuple(int(x[p]) for x in got) != want:
                fail("SW SPAN", spec, p, pairs[p], tuple(int(x[p]) for x in got), want)
            want_runs.append(gaps_want(h))
            want7 = want + (ST.count_columns(osc, h["a"].encode(), h["b"].encode()) if h else (0, 0))
            if tuple(int(x[p]) for x in got7) != want7:
                fail("SW STATS", spec, p, pairs[p], tuple(int(x[p]) for x in got7), want7)
        n["span"] += 12
        n["sw_stats"] += len(pairs)
        # ---- SW identity counts on the same batch: sw_score's three byte for byte, sw_stats' two counts and its pos + len
        got5 = ctx.sw_counts(batch, sc)
        if any(x.tobytes() != y.tobytes() for x, y in zip(got5, counts_view(got7))) or any(x.tobytes() != y.tobytes() for x, y in zip(got5[:3], (s, ea, eb))):
            fail("SW COUNTS", spec, pairs, [tuple(int(x[p]) for x in got5) for p in range(len(pairs))])
        n["sw_counts"] += len(pairs)
        # ---- SW gap runs on the same batch: sw_score's three byte for byte, the '-' runs of the oracle's strings
        gaps5 = ctx.sw_gaps(batch, sc)
        if gaps_got(gaps5) != want_runs or any(x.tobytes() != y.tobytes() for x, y in zip(gaps5[:3], (s, ea, eb))):
            fail("SW GAPS", spec, pairs, gaps_got(gaps5), want_runs)
        n["sw_gaps"] += len(pairs)

        # ---- NW statistics: the columns of the oracle's strings, counted on the host
        if nw_ok:
            got = ST.got_stats(ctx.nw_stats(batch, sc))
            runs = ST.got_stats(ctx.nw_gaps(batch, sc))       # NW gap runs on the same batch: the '-' runs of the same strings
            for p, (a, b) in enumerate(pairs):
                rc, score, ra, rb = O.oracle_nw_traceback(osc, a, b, *fills[0, p])
                want = (score,) + ST.count_columns(osc, ra, rb) if rc == 0 else None
                if got[p] != want:
                    fail("NW STATS", spec, p, pairs[p], got[p], want)
                want = (score, dash_runs(ra), dash_runs(rb)) if rc == 0 else None
                if runs[p] != want:
                    fail("NW GAPS", spec, p, pairs[p], runs[p], want)
            n["stats"] += len(pairs)
            n["nw_gaps"] += len(pairs)

        # ---- score matrices and the search over them: 4 queries x 6 targets taken from the pairs
        qi = [0, 3, 6, wide if wide >= 0 else 9]
        ti = [1, 2, 5, 7, 10, 11]
        queries, targets = [pairs[p][0] for p in qi], [pairs[p][1] for p in ti]
        q, t = W.seqset_from(queries), W.seqset_from(targets)
        k_top = (1, 3, 8)[int(v[11] % 3)]
        for is_sw in ((0, 1) if nw_ok else (1,)):
            dense = np.zeros((4, 6), np.int32), np.zeros((4, 6), np.uint32), np.zeros((4, 6), np.uint32)
            for i, a in enumerate(queries):
                for j, b in enumerate(targets):
                    rc, M, A, B = O.oracle_fill(osc, a, b, is_sw)
                    if rc != 0:
                        fail("ORACLE", spec, (a, b))
                    if is_sw:
                        dense[0][i, j], dense[1][i, j], dense[2][i, j] = best_cell(M, len(a), len(b))
                    else:
                        dense[0][i, j] = max(M[-1], A[-1], B[-1])
            if is_sw:
                got = ctx.sw_score_cross(q, t, sc)
            else:
                got = (ctx.nw_score_cross(q, t, sc), dense[1], dense[2])
            if not all(np.array_equal(g, w) for g, w in zip(got, dense)):
                fail("SW CROSS" if is_sw else "NW CROSS", spec, queries, targets, [g.tolist() for g in got], [w.tolist() for w in dense])
            n["cross"] += 24
            min_score = int(np.median(dense[0][int(v[12] % 4)])) + int(v[13] % 3) - 1     # around one row's median
            n_hits, hits = (ctx.sw_score_search if is_sw else ctx.nw_score_search)(q, t, sc, k_top, min_score=min_score)
            for i, (tg, ws, wa, wb) in enumerate(top_k(*dense, k_top, min_score)):
                h = hits[i, :int(n_hits[i])]
                if not (int(n_hits[i]) == len(tg) and np.array_equal(h["target"], tg) and np.array_equal(h["score"], ws)
                        and np.array_equal(h["end_a"], wa) and np.array_equal(h["end_b"], wb)):
                    fail("SW SEARCH" if is_sw else "NW SEARCH", spec, "k", k_top, "min_score", min_score, "query", i, queries[i], targets,
                         h.tolist(), (tg.tolist(), ws.tolist()))
            n["search"] += 4
            if not is_sw:
                # ---- the same sets' statistics matrices: nw_stats on the explicit batch, the oracle's scores
                want = tuple(x.reshape(4, 6) for x in ctx.nw_stats(W.cross_batch(q, t), sc))
                got = ctx.nw_stats_cross(q, t, sc)
                if not (all(np.array_equal(g, w) for g, w in zip(got, want)) and np.array_equal(got[0], dense[0])):
                    fail("NW STATS CROSS", spec, queries, targets, [g.tolist() for g in got], [w.tolist() for w in want])
                n["stats_cross"] += 24
                # ---- and their gap-run matrices: nw_gaps on the explicit batch (held to the oracle's strings above)
                want = tuple(x.reshape(4, 6) for x in ctx.nw_gaps(W.cross_batch(q, t), sc))
                got = ctx.nw_gaps_cross(q, t, sc)
                if not (all(np.array_equal(g, w) for g, w in zip(got, want)) and np.array_equal(got[0], dense[0])):
                    fail("NW GAPS CROSS", spec, queries, targets, [g.tolist() for g in got], [w.tolist() for w in want])
                n["nw_gaps_cross"] += 24
                continue
            # ---- the same sets' span matrices and search with spans: sw_span on the explicit batch, the oracle's best cells
            want = tuple(x.reshape(4, 6) for x in ctx.sw_span(W.cross_batch(q, t), sc))
            got = ctx.sw_span_cross(q, t, sc)
            if not (all(np.array_equal(g, w) for g, w in zip(got, want)) and np.array_equal(got[0], dense[0])
                    and np.array_equal(got[1] + got[3], dense[1]) and np.array_equal(got[2] + got[4], dense[2])):
                fail("SW SPAN CROSS", spec, queries, targets, [g.tolist() for g in got], [w.tolist() for w in want])
            n["span_cross"] += 24
            # ---- the same sets' SW statistics matrices: sw_stats on the explicit batch, the span matrices just checked
            want7 = tuple(x.reshape(4, 6) for x in ctx.sw_stats(W.cross_batch(q, t), sc))
            got7 = ctx.sw_stats_cross(q, t, sc)
            if not (all(np.array_equal(g, w) for g, w in zip(got7, want7)) and all(np.array_equal(g, w) for g, w in zip(got7[:5], got))):
                fail("SW STATS CROSS", spec, queries, targets, [g.tolist() for g in got7], [w.tolist() for w in want7])
            n["sw_stats_cross"] += 24
            n_span, span_hits = ctx.sw_span_search(q, t, sc, k_top, min_score=min_score)
            for i in range(4):
                h, hs = span_hits[i, :int(n_span[i])], hits[i, :int(n_hits[i])]
                if not (int(n_span[i]) == int(n_hits[i]) and np.array_equal(h["target"], hs["target"]) and np.array_equal(h["score"], hs["score"])
                        and all(np.array_equal(h[name], w[i][h["target"]]) for name, w in zip(("pos_a", "pos_b", "len_a", "len_b"), want[1:]))):
                    fail("SW SPAN SEARCH", spec, "k", k_top, "min_score", min_score, "query", i, queries[i], targets, h.tolist(), hs.tolist())
            n["span_search"] += 4

        # ---- alignments of any length
        rows = (1, 3, 17, 64, 0)[int(v[14] % 5)]
        with ctx.options(long_block_rows=rows):
            if nw_ok:
                got = ctx.nw_align_long(batch, sc)
                for p, (a, b) in enumerate(pairs):
                    rc, s_, ra, rb = O.oracle_nw_traceback(osc, a, b, *fills[0, p])
                    if rc != 0 or got[p] != (s_, ra, rb):
                        fail("NW LONG", spec, "long_block_rows", rows, p, pairs[p], got[p], (s_, ra, rb))
            got = ctx.sw_align_long(batch, sc, thr)
            for p, (a, b) in enumerate(pairs):
                rc, want = O.oracle_sw_hits(osc, a, b, *fills[1, p], thr, 1)
                if rc != 0 or got[p] != want:
                    fail("SW LONG", spec, "long_block_rows", rows, "thr", thr, p, pairs[p], got[p], want)
        n["long"] += 12 * (1 + nw_ok)

        # ---- banded NW: at most 4 pairs of at most 260 x 260, w in 0 .. 40 (the reference is Python: ~3e5 band cells a trial)
        if nw_ok:
            n["nw_trials"] += 1
            small = [p for p in range(12) if max(len(pairs[p][0]), len(pairs[p][1])) <= 260][:4]
            sub = [pairs[p] for p in small]
            bands = [int((v[3] + 7 * p) % 41) for p in small]
            both = [BL.expected_both(osc, a, b, w) for (a, b), w in zip(sub, bands)]
            if sub:
                got = ctx.nw_score_banded(W.from_pairs(sub), sc, bands)
                if [int(x) for x in got] != [x[0] for x in both]:
                    fail("BAND SCORE", spec, sub, bands, [int(x) for x in got], [x[0] for x in both])
                # ---- banded NW statistics on the same pairs and bands
                kept, lost = nw_stats_banded_check("BAND NW STATS", ctx.nw_stats_banded, None, spec, sub, bands, both, 0)
                n["stats_banded"] += kept
                n["stats_banded_none"] += lost
                # ---- banded NW gap runs on the same pairs and bands: the '-' runs of the same walks, the same pairs without one
                n["nw_gaps_banded"] += nw_stats_banded_check("BAND NW GAPS", ctx.nw_gaps_banded, None, spec, sub, bands, both, 0,
                                                             lambda ra, rb: (dash_runs(ra), dash_runs(rb)))[0]
                none = [k for k, x in enumerate(both) if x[1] is None]
                if none:            # no alignment inside the band: the call says so and names the lowest such pair
                    try:
                        ctx.nw_align_banded(W.from_pairs(sub), sc, bands)
                        fail("BAND NONE", spec, sub, bands, none, "no error")
                    except S.SeqAlignError as e:
                        if e.code != S.E_TRACEBACK or f"pair {none[0]}:" not in str(e):
                            fail("BAND NONE", spec, sub, bands, none, str(e))
                    n["banded_none"] += len(none)
                    keep = [k for k in range(len(sub)) if k not in none]
                    sub, bands, both = [sub[k] for k in keep], [bands[k] for k in keep], [both[k] for k in keep]
            if sub:
                got = ctx.nw_align_banded(W.from_pairs(sub), sc, bands)
                if got != [x[1] for x in both]:
                    fail("BAND ALIGN", spec, sub, bands, got, [x[1] for x in both])
            n["banded"] += len(sub)

        # ---- banded SW hit spans: at most 4 pairs of at most 260 x 260, bounds on either side of the pair's diagonals, up to 140 wide
        small = [p for p in range(12) if max(len(pairs[p][0]), len(pairs[p][1])) <= 260][:4]
        if small:
            sub = [pairs[p] for p in small]
            lo = [int((v[5] + 31 * p) % 300) - 200 for p in small]
            hi = [lo[k] + int((v[6] + 17 * p) % 140) for k, p in enumerate(small)]
            hits = [BS.expected(osc, a, b, lo[k], hi[k], 1)[1] for k, (a, b) in enumerate(sub)]
            want = [(h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0) for h in hits]
            res = ctx.sw_span_banded(W.from_pairs(sub), sc, lo, hi)
            got = [tuple(int(x[k]) for x in res) for k in range(len(sub))]
            if got != want:
                fail("SW SPAN BANDED", spec, sub, lo, hi, got, want)
            n["span_banded"] += len(sub)
            # ---- banded SW statistics on the same pairs and bounds: the oracle's banded hit and its counted strings
            want = [tuple(w) + ST.count_columns(osc, h["a"].encode(), h["b"].encode()) if h else (0,) * 7 for w, h in zip(want, hits)]
            res = ctx.sw_stats_banded(W.from_pairs(sub), sc, lo, hi)
            got = [tuple(int(x[k]) for x in res) for k in range(len(sub))]
            if got != want:
                fail("SW STATS BANDED", spec, sub, lo, hi, got, want)
            n["sw_stats_banded"] += len(sub)
            # ---- banded SW identity counts on the same pairs and bounds: sw_score_banded's three, sw_stats_banded's counts
            res5 = ctx.sw_counts_banded(W.from_pairs(sub), sc, lo, hi)
            if any(x.tobytes() != y.tobytes() for x, y in zip(res5, counts_view(res))) or \
                    any(x.tobytes() != y.tobytes() for x, y in zip(res5[:3], ctx.sw_score_banded(W.from_pairs(sub), sc, lo, hi))):
                fail("SW COUNTS BANDED", spec, sub, lo, hi, [tuple(int(x[k]) for x in res5) for k in range(len(sub))], want)
            n["sw_counts_banded"] += len(sub)
            # ---- banded SW gap runs on the same pairs and bounds: sw_counts_banded's three, the '-' runs of the oracle's banded hit
            gaps5 = ctx.sw_gaps_banded(W.from_pairs(sub), sc, lo, hi)
            if gaps_got(gaps5) != [gaps_want(h) for h in hits] or any(x.tobytes() != y.tobytes() for x, y in zip(gaps5[:3], res5[:3])):
                fail("SW GAPS BANDED", spec, sub, lo, hi, gaps_got(gaps5), [gaps_want(h) for h in hits])
            n["sw_gaps_banded"] += len(sub)

        # ---- the wide banded calls: two small pairs (the narrow calls must agree) and one of 1 025 .. 1 624 columns whose band is
        # 700 .. 1 500 diagonals wide, under a random strip width
        if wide_calls:
            small = [p for p in range(12) if max(len(pairs[p][0]), len(pairs[p][1])) <= 260][:2]
            la = int(1025 + v[10] % 600)
            a = rand(la)
            long_pair = (a, BL.mutate(random.Random(int(v[11])), a, 0.08)[:la + 40])
            sub = [pairs[p] for p in small] + [long_pair]
            cols = (0, 64, 128, 256, 512)[int(v[12] % 5)]
            half = int(350 + v[13] % 400)                      # the long pair: about 2 * half + 1 diagonals
            wb = W.from_pairs(sub)
            with ctx.options(band_strip_cols=cols):
                if nw_ok:
                    bands = [int((v[3] + 7 * p) % 41) for p in small] + [half]
                    both = [BL.expected_both(osc, a, b, w) for (a, b), w in zip(sub, bands)]
                    got = ctx.nw_score_banded_wide(wb, sc, bands)
                    if [int(x) for x in got] != [x[0] for x in both]:
                        fail("WIDE BAND SCORE", spec, "cols", cols, sub, bands, [int(x) for x in got], [x[0] for x in both])
                    if small and not np.array_equal(got[:len(small)], ctx.nw_score_banded(W.from_pairs(sub[:len(small)]), sc, bands[:len(small)])):
                        fail("WIDE / NARROW BAND SCORE", spec, "cols", cols, sub, bands)
                    keep = [k for k, x in enumerate(both) if x[1] is not None]
                    if keep:
                        got = ctx.nw_align_banded_wide(W.from_pairs([sub[k] for k in keep]), sc, [bands[k] for k in keep])
                        if got != [both[k][1] for k in keep]:
                            fail("WIDE BAND ALIGN", spec, "cols", cols, [sub[k] for k in keep], [bands[k] for k in keep], got)
                    n["banded_wide"] += len(keep)
                    # ---- wide banded NW statistics on the same pairs and bands, and the narrow call's bytes on the small pairs
                    n["stats_banded_wide"] += nw_stats_banded_check("WIDE BAND NW STATS", ctx.nw_stats_banded_wide, ctx.nw_stats_banded, spec, sub, bands,
                                                                    both, len(small))[0]
                    n["nw_gaps_banded_wide"] += nw_stats_banded_check("WIDE BAND NW GAPS", ctx.nw_gaps_banded_wide, ctx.nw_gaps_banded, spec, sub, bands,
                                                                      both, len(small), lambda ra, rb: (dash_runs(ra), dash_runs(rb)))[0]
                shift = int(v[14] % 300) - 150
                lo = [int(v[5] % 80) - 60] * len(small) + [shift - half]
                hi = [lo[k] + int(v[6] % 90) for k in range(len(small))] + [shift + half]
                want = [BS.expected(osc, a, b, lo[k], hi[k], thr) for k, (a, b) in enumerate(sub)]
                s, ea, eb = ctx.sw_score_banded_wide(wb, sc, lo, hi)
                cells = [(int(s[k]), int(ea[k]), int(eb[k])) for k in range(len(sub))]
                if cells != [x[0] for x in want]:
                    fail("WIDE BAND SW SCORE", spec, "cols", cols, sub, lo, hi, cells, [x[0] for x in want])
                got = ctx.sw_align_banded_wide(wb, sc, lo, hi, thr)
                if got != [[x[1]] if x[1] else [] for x in want]:
                    fail("WIDE BAND SW ALIGN", spec, "cols", cols, "thr", thr, sub, lo, hi, got, [x[1] for x in want])
                if small and got[:len(small)] != ctx.sw_align_banded(W.from_pairs(sub[:len(small)]), sc, lo[:len(small)], hi[:len(small)], thr):
                    fail("WIDE / NARROW BAND SW ALIGN", spec, "cols", cols, sub, lo, hi)
                n["banded_wide"] += len(sub)
                # ---- wide banded SW hit spans on the same pairs and bounds: the fields of the oracle's banded hit at min_score = 1
                # (the hit found above where it reached thr), and the narrow call's bytes on the small pairs
                hits1 = [x[1] if x[1] else BS.expected(osc, a, b, lo[k], hi[k], 1)[1] for k, ((a, b), x) in enumerate(zip(sub, want))]
                want5 = [(h["score"], h["pos_a"], h["pos_b"], h["len_a"], h["len_b"]) if h else (0, 0, 0, 0, 0) for h in hits1]
                res = ctx.sw_span_banded_wide(wb, sc, lo, hi)
                got5 = [tuple(int(x[k]) for x in res) for k in range(len(sub))]
                if got5 != want5:
                    fail("WIDE BAND SW SPAN", spec, "cols", cols, sub, lo, hi, got5, want5)
                if small:
                    narrow = ctx.sw_span_banded(W.from_pairs(sub[:len(small)]), sc, lo[:len(small)], hi[:len(small)])
                    if any(x[:len(small)].tobytes() != y.tobytes() for x, y in zip(res, narrow)):
                        fail("WIDE / NARROW BAND SW SPAN", spec, "cols", cols, sub, lo, hi)
                n["span_banded_wide"] += len(sub)
                # ---- wide banded SW statistics on the same pairs and bounds: that hit and its counted strings, and the narrow
                # call's bytes on the small pairs
                want7 = [w5 + (ST.count_columns(osc, h["a"].encode(), h["b"].encode()) if h else (0, 0)) for w5, h in zip(want5, hits1)]
                res = ctx.sw_stats_banded_wide(wb, sc, lo, hi)
                got7 = [tuple(int(x[k]) for x in res) for k in range(len(sub))]
                if got7 != want7:
                    fail("WIDE BAND SW STATS", spec, "cols", cols, sub, lo, hi, got7, want7)
                if small:
                    narrow = ctx.sw_stats_banded(W.from_pairs(sub[:len(small)]), sc, lo[:len(small)], hi[:len(small)])
                    if any(x[:len(small)].tobytes() != y.tobytes() for x, y in zip(res, narrow)):
                        fail("WIDE / NARROW BAND SW STATS", spec, "cols", cols, sub, lo, hi)
                n["sw_stats_banded_wide"] += len(sub)
                # ---- wide banded SW identity counts on the same pairs and bounds: sw_score_banded_wide's three (checked against
                # the oracle above), sw_stats_banded_wide's counts, and the narrow call's bytes on the small pairs
                res5 = ctx.sw_counts_banded_wide(wb, sc, lo, hi)
                if any(x.tobytes() != y.tobytes() for x, y in zip(res5, counts_view(res))) or any(x.tobytes() != y.tobytes() for x, y in zip(res5[:3], (s, ea, eb))):
                    fail("WIDE BAND SW COUNTS", spec, "cols", cols, sub, lo, hi, [tuple(int(x[k]) for x in res5) for k in range(len(sub))], want7)
                if small:
                    narrow = ctx.sw_counts_banded(W.from_pairs(sub[:len(small)]), sc, lo[:len(small)], hi[:len(small)])
                    if any(x[:len(small)].tobytes() != y.tobytes() for x, y in zip(res5, narrow)):
                        fail("WIDE / NARROW BAND SW COUNTS", spec, "cols", cols, sub, lo, hi)
                n["sw_counts_banded_wide"] += len(sub)
                # ---- wide banded SW gap runs on the same pairs and bounds: sw_counts_banded_wide's three, the '-' runs of the
                # oracle's banded hit at min_score = 1, and the narrow call's bytes on the small pairs
                gaps5 = ctx.sw_gaps_banded_wide(wb, sc, lo, hi)
                if gaps_got(gaps5) != [gaps_want(h) for h in hits1] or any(x.tobytes() != y.tobytes() for x, y in zip(gaps5[:3], res5[:3])):
                    fail("WIDE BAND SW GAPS", spec, "cols", cols, sub, lo, hi, gaps_got(gaps5), [gaps_want(h) for h in hits1])
                if small:
                    narrow = ctx.sw_gaps_banded(W.from_pairs(sub[:len(small)]), sc, lo[:len(small)], hi[:len(small)])
                    if any(x[:len(small)].tobytes() != y.tobytes() for x, y in zip(gaps5, narrow)):
                        fail("WIDE / NARROW BAND SW GAPS", spec, "cols", cols, sub, lo, hi)
                n["sw_gaps_banded_wide"] += len(sub)
        n["trials"] += 1

    if srng is not None:
        print(f"fuzz_calls scale up to {scale}: {n['redraws']} factors redrawn in {n['redrawn_trials']} of {n['trials']} trials "
              f"({n['redrawn_trials'] / max(1, n['trials']):.1%} of the trials)", flush=True)
    print(f"fuzz_calls ok: {n['trials']} random scorings x batches ({n['nw_trials']} in NW's domain, {n['wide']} pairs over 1 024 columns); "
          f"{n['score']} scores, {n['span']} hit spans, {n['span_banded']} banded hit spans, {n['sw_stats_banded']} banded SW statistics, {n['cross']} cross cells, {n['search']} searches, {n['span_cross']} span cross cells, {n['span_search']} span searches, {n['stats']} NW and {n['sw_stats']} SW statistics, {n['stats_cross']} NW and {n['sw_stats_cross']} SW statistics cross cells, {n['long']} long alignments, {n['banded']} banded "
          f"alignments (+ {n['banded_none']} with none in their band), {n['stats_banded']} banded NW statistics (+ {n['stats_banded_none']} with none), {n['banded_wide']} wide banded results, {n['span_banded_wide']} wide banded hit spans, "
          f"{n['stats_banded_wide']} wide banded NW and {n['sw_stats_banded_wide']} wide banded SW statistics identical to the oracle; "
          f"{n['sw_counts']} SW identity counts, {n['sw_counts_banded']} banded and {n['sw_counts_banded_wide']} wide banded identical to sw_stats* and sw_score*; "
          f"{n['sw_gaps']} SW gap runs, {n['sw_gaps_banded']} banded and {n['sw_gaps_banded_wide']} wide banded identical to the oracle's strings; "
          f"{n['nw_gaps']} NW gap runs, {n['nw_gaps_cross']} cross cells, {n['nw_gaps_banded']} banded and {n['nw_gaps_banded_wide']} wide banded identical to the oracle's strings "
          f"(seed {seed})", flush=True)
    return n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--trials", type=int, default=1 << 60)
    ap.add_argument("--no-wide", action="store_true", help="leave the wide banded calls out")
    ap.add_argument("--scale", type=int, default=1, help="multiply every trial's scoring by a drawn factor of up to this")
    args = ap.parse_args()
    run(args.seconds, args.seed, args.trials, wide_calls=not args.no_wide, scale=args.scale)
