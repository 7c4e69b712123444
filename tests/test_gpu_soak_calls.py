"""GPU tier: a seeded slice of seq-align_amd/tools/fuzz_calls.py, as test_gpu_soak.py runs one of fuzz_e2e.py.

Random scorings (penalties, the five flags, case sensitivity, a wildcard, mutations that differ by direction) x random,
related and tandem-repeat pairs, some wider than 1 024 columns: the score, cross, search, long and banded calls against the
oracle and bandlib.  Bounded by trial count, so the cases are the same on every machine; the wall-clock cap is a backstop.
A mismatch raises SystemExit(1) inside the tool with the failing case printed.
"""
import importlib.util
from pathlib import Path

import pytest

import seqalign_amd as S

pytestmark = pytest.mark.gpu

TOOLS = Path(__file__).resolve().parent.parent / "seq-align_amd" / "tools"


@pytest.fixture(scope="module")
def ctx():
    with S.Context(0) as c:
        yield c


@pytest.mark.parametrize("seed", [20261018, 11])
def test_fuzz_calls_slice(ctx, seed):
    spec = importlib.util.spec_from_file_location("soak_fuzz_calls", TOOLS / "fuzz_calls.py")
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    before = ctx.get_option("long_block_rows")
    try:
        r = fz.run(seconds=40.0, seed=seed, max_trials=40, ctx=ctx)
    except SystemExit as e:
        pytest.fail(f"fuzz_calls mismatch (seed {seed}); the failing case is in the captured output (exit {e.code})")
    assert ctx.get_option("long_block_rows") == before
    assert r["trials"] >= 15, r                    # 40 on a healthy machine; the wall-clock cap is a backstop only
    for family in ("score", "cross", "search", "long", "banded", "nw_trials", "wide"):
        assert r[family] > 0, (family, r)
    assert r["score"] == 12 * (r["trials"] + r["nw_trials"]) == r["long"] and r["search"] == 4 * (r["trials"] + r["nw_trials"]), r


SCALE = 1 << 23


def test_fuzz_calls_slice_at_large_scores(ctx):
    """The same slice with every trial's scoring multiplied by a drawn factor of 2^8 .. 2^23 (fuzz_calls.run's scale): cells
    up to 2^31.  A factor under which the exact peak leaves int32, or which the documented magnitude bound refuses, is drawn
    again; at most one trial in four may need that (tests/test_magnitude_argument_cpu.py checks the share on the CPU)."""
    spec = importlib.util.spec_from_file_location("soak_fuzz_calls", TOOLS / "fuzz_calls.py")
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    try:
        r = fz.run(seconds=40.0, seed=20261019, max_trials=40, ctx=ctx, scale=SCALE)
    except SystemExit as e:
        pytest.fail(f"fuzz_calls mismatch at scale {SCALE}; the failing case is in the captured output (exit {e.code})")
    assert r["trials"] >= 15, r
    assert 4 * r["redrawn_trials"] <= r["trials"], r
    for family in ("score", "cross", "search", "long", "banded", "nw_trials", "wide", "span", "span_banded"):
        assert r[family] > 0, (family, r)


WIDE_TRIALS = 12


def test_fuzz_calls_slice_with_the_wide_banded_calls(ctx):
    """A short slice with wide_calls=True: the *_banded_wide calls -- the score, align and span forms and the NW and SW
    statistics -- on two small pairs (where each must return its narrow call's bytes) and one pair of 1 025 .. 1 624 columns
    whose band is 700 .. 1 500 diagonals wide, under a random strip width; the narrow banded NW statistics run in every slice.
    12 trials.  Their Python and oracle reference side alone -- the draws of this recipe, the fills, walks and banded
    definitions each block computes, no device: 1.7 s for the 12 trials (0.10 to 0.24 s a trial, of which the wide block
    0.08 to 0.16 s)."""
    spec = importlib.util.spec_from_file_location("soak_fuzz_calls", TOOLS / "fuzz_calls.py")
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    before = ctx.get_option("band_strip_cols"), ctx.get_option("long_block_rows")
    try:
        r = fz.run(seconds=40.0, seed=20261021, max_trials=WIDE_TRIALS, ctx=ctx, wide_calls=True)
    except SystemExit as e:
        pytest.fail(f"fuzz_calls mismatch with the wide calls; the failing case is in the captured output (exit {e.code})")
    assert (ctx.get_option("band_strip_cols"), ctx.get_option("long_block_rows")) == before
    assert r["trials"] == WIDE_TRIALS, r
    for family in ("stats_banded", "stats_banded_wide", "sw_stats_banded_wide", "banded_wide", "span_banded_wide", "nw_trials"):
        assert r[family] > 0, (family, r)
