"""GPU tier: where the banded calls cut a batch into chunks -- seqalign_{nw,sw}_{score,align}_banded and their wide forms
(sa_batch_band.hip).  The span and statistics calls pin their cut in their own files; this one does it for the other eight.

A chunk closes before the pair that would take its device bytes over the budget (include/seqalign_hip.h).  A pair's bytes:
    nw_score_banded   len_a + len_b + 64
    sw_score_banded   len_a + len_b + 80
    nw_align_banded   12 (len_b + 1) width + 3 (len_a + len_b) + 96
    sw_align_banded   12 rows width + 3 (len_a + len_b) + 128      rows: those with inner band cells (sa_band_sw_rows)
    the wide forms    ... + strips (8 width + 20) + 20             strips = max(1, ceil(len_a / band_strip_cols))
Every case builds its batch around that model at chunk_bytes = 1 MiB: the first chunk is filled to within a few bytes of the
budget, the second is missed by a few bytes by the pair that opens the third.  The model with the per-pair constant 16 bytes
smaller or larger cuts elsewhere (asserted on the CPU); the launch records -- one band_score / band_fill launch per width
class of a chunk, or per chunk in the wide forms, one band_walk per chunk -- must be the model's cut's.  Results must equal the
one-chunk call's, and the wide calls' the narrow ones'.  Last, a pair too large for the budget alone must be refused with the
model's bytes in the message, which holds the library to the formula and the constant to the byte."""
import random
from typing import NamedTuple

import numpy as np
import pytest

import bandlib as BL
import bandswlib as BS
import seqalign_amd as S
from seqalign_amd import workloads as W

pytestmark = pytest.mark.gpu

BUDGET = 1 << 20
COLS = 64                                                # band_strip_cols of the wide cases
LADDER = [64, 128, 192, 256, 320, 384, 512, 768, 1024]   # widths at which the columns per lane step up
LETTERS = np.frombuffer(b"ACGT", np.uint8)


class Mode(NamedTuple):
    name: str
    sw: bool
    align: bool
    const: int          # the fixed bytes per pair


MODES = {m.name: m for m in (Mode("nw_score", False, False, 64), Mode("sw_score", True, False, 80),
                             Mode("nw_align", False, True, 96), Mode("sw_align", True, True, 128))}


@pytest.fixture(scope="module")
def ctx():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device; there is no CPU fallback"
    with S.Context(0) as c:
        yield c


# ---------------------------------------------------------------- the model --
# a pair is (len_a, len_b, band): band = w of the NW calls, (diag_lo, diag_hi) of the SW calls
def geometry(mode, spec):
    """(width, cells of one stored matrix) of a pair."""
    la, lb, band = spec
    if not mode.sw:
        width = BL.width_of(la, lb, band)
        return width, (lb + 1) * width
    d_lo, d_hi = BS.clip(la, lb, *band)
    j0, j1 = (1 - d_hi if d_hi < 0 else 1), min(la - d_lo, lb)
    return d_hi - d_lo + 1, max(0, j1 - j0 + 1) * (d_hi - d_lo + 1)


def bytes_of(mode, spec, cols):
    """A pair's device bytes without the constant; cols: the strip columns of a wide call, 0 for the narrow one."""
    la, lb, _ = spec
    width, cells = geometry(mode, spec)
    wide = max(1, -(-la // cols)) * (8 * width + 20) + 20 if cols else 0
    return wide + (12 * cells + 3 * (la + lb) if mode.align else la + lb)


def cut(needs):
    chunks, used = [[]], 0
    for k, need in enumerate(needs):
        assert need <= BUDGET
        if chunks[-1] and used + need > BUDGET:
            chunks.append([])
            used = 0
        chunks[-1].append(k)
        used += need
    return chunks


def class_of(width):
    return next(k for k, edge in enumerate(LADDER) if width <= edge)


def launches(mode, cols, specs, chunks):
    """band_score / band_fill launches of a call that is cut into `chunks`."""
    if cols:
        return len(chunks)
    return sum(len({class_of(geometry(mode, specs[k])[0]) for k in c}) for c in chunks)


def pinned(mode, cols, parts, cands):
    """parts[0] + [fit] + parts[1] + [over] + parts[2]: `fit` the candidate that fills the first chunk best, `over` the
    one that misses the second by least.  Returns the pairs and their cut, three chunks, after asserting that the model with
    16 bytes less or more per pair cuts elsewhere."""
    need = lambda s: bytes_of(mode, s, cols) + mode.const
    sized = [(need(c), c) for c in cands]
    rooms = [BUDGET - sum(need(s) for s in part) for part in parts]
    assert min(rooms) > 0, rooms
    fit = max((x for x in sized if x[0] <= rooms[0]), key=lambda x: x[0])
    over = min((x for x in sized if x[0] > rooms[1]), key=lambda x: x[0])
    specs = parts[0] + [fit[1]] + parts[1] + [over[1]] + parts[2]
    base = [bytes_of(mode, s, cols) for s in specs]
    chunks = cut([x + mode.const for x in base])
    assert [len(c) for c in chunks] == [len(parts[0]) + 1, len(parts[1]), 1 + len(parts[2])], [len(c) for c in chunks]
    print(mode.name, "cols", cols, "pairs per chunk", [len(c) for c in chunks], "chunk 1 is", rooms[0] - fit[0],
          "bytes short of the budget, chunk 2 is missed by", over[0] - rooms[1])
    for delta in (-16, 16):
        assert cut([x + mode.const + delta for x in base]) != chunks, delta
    return specs, chunks


# ---------------------------------------------------------------- batches and calls --
def batch_of(seed, specs):
    """Per pair a random seq_a and a seq_b that is its copy with 5 % of the letters changed (none in pairs of 1 000
    letters and more: self-pairs), each cut to its length."""
    g = np.random.default_rng(seed)
    pairs = []
    for la, lb, _ in specs:
        n = max(la, lb)
        x = g.integers(0, 4, n)
        y = np.where(g.random(n) < (0.05 if n < 1000 else 0.0), (x + 1) % 4, x)
        pairs.append((LETTERS[x[:la]].tobytes(), LETTERS[y[:lb]].tobytes()))
    return W.from_pairs(pairs)


def call(ctx, mode, wide, batch, sc, specs):
    """(the result in a form that compares with ==, the launch records)."""
    fn = getattr(ctx, mode.name + "_banded" + ("_wide" if wide else ""))
    if mode.sw:
        lo, hi = [s[2][0] for s in specs], [s[2][1] for s in specs]
        res = fn(batch, sc, lo, hi, 1) if mode.align else fn(batch, sc, lo, hi)
    else:
        res = fn(batch, sc, [s[2] for s in specs])
    if not mode.align:
        res = tuple(r.tobytes() for r in (res if mode.sw else (res,)))
    return res, ctx.last_call()


def records(mode, n_launches, n_items, n_chunks, n):
    if mode.align:
        return {"band_fill": (n_launches, n_items), "band_walk": (n_chunks, n)}
    return {"band_score": (n_launches, n_items)}


def run_case(ctx, mode, cols, specs, chunks, seed):
    """The narrow call in one chunk; then the call under test (cols: its wide form) in one chunk and in the model's."""
    sc = S.make_scoring({"init": [*([2, -3, -4, -1] if mode.sw else [1, -2, -4, -1]), 0, 0, 0, 0, 0, 0]})
    batch = batch_of(seed, specs)
    n = len(specs)
    everything = [list(range(n))]
    one, info = call(ctx, mode, False, batch, sc, specs)
    items = n
    assert info == records(mode, launches(mode, 0, specs, everything), n, 1, n), info
    with ctx.options(band_strip_cols=cols):
        if cols:
            narrow = one
            one, info = call(ctx, mode, True, batch, sc, specs)
            items = info["band_fill" if mode.align else "band_score"][1]     # the strips that sweep a row
            assert info == records(mode, 1, items, 1, n) and one == narrow, info
        with ctx.options(chunk_bytes=BUDGET):
            got, info = call(ctx, mode, bool(cols), batch, sc, specs)
    assert info == records(mode, launches(mode, cols, specs, chunks), items, len(chunks), n), info
    assert got == one
    # the records show a cut's chunks and width classes, not every pair that changes sides: a pair that does not fit the
    # budget alone is refused with its bytes named, and those are the model's to the byte
    alone = (700, 700, (-64, 64) if mode.sw else 64) if mode.align else (600000, 600000, (-1, 1) if mode.sw else 1)
    need = bytes_of(mode, alone, cols) + mode.const
    assert need > BUDGET
    with ctx.options(band_strip_cols=cols, chunk_bytes=BUDGET):
        with pytest.raises(S.SeqAlignError) as e:
            call(ctx, mode, bool(cols), batch_of(seed, [specs[0], alone]), sc, [specs[0], alone])
    assert e.value.code == S.E_NOMEM and f"pair 1: {need} bytes of device memory needed" in str(e.value), (need, str(e.value))


# ---------------------------------------------------------------- 1. the score calls --
def self_cands(mode):
    """The score calls' candidates: self-pairs of 64 .. 40 000 letters with len_b = len_a or one less under a band of three or
    four diagonals, 130 bytes to 80 KB and more, every byte count of the narrow calls among them."""
    return [(la, lb, (-1, 1) if mode.sw else 1) for la in range(64, 40000) for lb in (la, la - 1)]


def score_parts(mode, rng):
    """60 pairs over the nine width classes in three parts of 20, each with 16, 16 and 14 self-pairs of 30 000 letters
    (60 064 or 60 080 bytes: about 69 KB of a MiB are left to the fitted pair); and the candidates."""
    widths = [1, 2, 64, 65, 128, 130, 192, 200, 256, 300, 320, 350, 384, 400, 512, 600, 768, 800, 1024, 1000]
    parts = []
    for part in range(3):
        specs = []
        for width in widths:
            if mode.sw:
                first = rng.randrange(-40, 10)
                specs.append((first + width + 60, rng.randrange(130, 180), (first, first + width - 1)))
            else:
                la = max(150, width) + rng.randrange(0, 40)
                lb = la - (width + 1) % 2                  # width = |len_a - len_b| + 2 w + 1
                specs.append((la, lb, BL.w_for_width(la, lb, width)))
            assert geometry(mode, specs[-1])[0] == width
        specs += [(30000, 30000, (-3, 3) if mode.sw else 3)] * (16 if part < 2 else 14)   # the third chunk opens with the pair that missed
        rng.shuffle(specs)
        parts.append(specs)
    return parts, self_cands(mode)


@pytest.mark.parametrize("name", ["nw_score", "sw_score"])
def test_score_calls_cut_at_the_sequences_bytes_and_the_constant(ctx, name):
    mode = MODES[name]
    parts, cands = score_parts(mode, random.Random(len(name) + mode.const))
    specs, chunks = pinned(mode, 0, parts, cands)
    small = [k for k, s in enumerate(specs) if s[0] < 30000 and s[2] not in (1, (-1, 1))]
    assert len(small) == 60 and {class_of(geometry(mode, specs[k])[0]) for k in small} == set(range(9))
    run_case(ctx, mode, 0, specs, chunks, 101)


# ---------------------------------------------------------------- 2. the align calls, and the wide forms --
def small_spec(mode, rng, la=None, w=None):
    """100 .. 200 letters a side, three letters apart at most, at most 64 diagonals on either side: widths up to 132."""
    la = la or rng.randrange(100, 201)
    lb = la - rng.randrange(-3, 4)
    w = rng.randrange(0, 65) if w is None else w
    return (la, lb, (-w - rng.randrange(0, 3), w) if mode.sw else w)


def small_cands(mode):
    rng = random.Random(5)
    return sorted({small_spec(mode, rng, la, w) for la in range(100, 201) for w in range(65) for _ in range(7)})


def drawn_parts(mode, cols, rng, big=(), leave=160 << 10):
    """Three parts of small pairs, each drawn until less than `leave` and no less than 4 KB of a MiB are left, beside `big`;
    the third leaves `leave` more, for the pair that missed the second chunk."""
    parts = []
    for part in range(3):
        specs = list(big)
        room = BUDGET - sum(bytes_of(mode, s, cols) + mode.const for s in specs)
        spare = leave if part == 2 else 0
        while room - spare > leave:
            s = small_spec(mode, rng)
            need = bytes_of(mode, s, cols) + mode.const
            if need <= room - spare - 4096:
                specs.append(s)
                room -= need
        rng.shuffle(specs)
        parts.append(specs)
    return parts


@pytest.mark.parametrize("name", ["nw_align", "sw_align"])
def test_align_calls_cut_at_the_band_cells_and_the_constant(ctx, name):
    mode = MODES[name]
    specs, chunks = pinned(mode, 0, drawn_parts(mode, 0, random.Random(mode.const)), small_cands(mode))
    assert len({class_of(geometry(mode, s)[0]) for s in specs}) >= 2       # widths up to 64, up to 128, a few above
    run_case(ctx, mode, 0, specs, chunks, 202)


@pytest.mark.parametrize("name", list(MODES))
def test_wide_calls_add_the_strips_bytes(ctx, name):
    """Strips of 64 columns: two to four per small pair.  The score calls' chunks hold seven self-pairs of 30 000 letters
    besides (469 strips, 11 or 7 diagonals: 111 KB and 96 KB), so that a hundred-odd small pairs fill them, not four hundred."""
    mode = MODES[name]
    rng = random.Random(mode.const + 1)
    if mode.align:
        specs, chunks = pinned(mode, COLS, drawn_parts(mode, COLS, rng), small_cands(mode))
    else:
        big = [(30000, 30000, (-3, 3) if mode.sw else 5)] * 7
        specs, chunks = pinned(mode, COLS, drawn_parts(mode, COLS, rng, big, 64 << 10), self_cands(mode))
    assert cut([bytes_of(mode, s, 0) + mode.const for s in specs]) != chunks  # the narrow call's bytes cut elsewhere
    run_case(ctx, mode, COLS, specs, chunks, 303)
