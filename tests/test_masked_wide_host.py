"""CPU suite for masked batches on the 128/256-query filter tile: `tavb_plan_masked_wide` against a restatement of its rule (and
`tavb_plan_masked` unchanged beside it), a numpy model of the mask words and bits every lane of a tile tests in both MFMA shapes checked
against the case table (tests/masked_wide_cases.py), the table's own claims from the float64 oracle, and the ABI."""

import itertools
import os

import numpy as np
import pytest

from tests import masked_wide_cases as mw
from typeagent_py_amd import _native

F16, F32 = _native.TAVB_F16, _native.TAVB_F32
MIB = 1 << 20
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the plan
def query_tile(nq: int, rows: int, n_cu: int = 256) -> int:
    """csrc/tavb_mfma_wide.hip::mfma_query_tile_for"""
    n128 = (nq + 127) // 128
    if (n128 & 1) and n128 <= 5:
        return 128
    wgs = ((nq + 255) // 256) * ((rows + 319) // 320)
    return 128 if wgs <= 4 * n_cu else 256


def rule_wide(nq, k, dim, dtype, allowed, span, min_bytes, pct) -> bool:
    if dtype != F16 or not (0 < dim <= 16384 and 1 <= k <= 256):
        return False
    if nq < 65 or allowed * dim * 2 < min_bytes:
        return False
    qt = query_tile(nq, span)
    return -(-nq // 8) * allowed * 100 >= -(-nq // qt) * span * pct


def rule_tile(nq, k, dim, dtype, allowed, span, min_bytes, pct) -> bool:
    """tavb_plan_masked as it was"""
    f32 = dtype == F32
    row_bytes = dim * (4 if f32 else 2)
    if dim <= 0 or row_bytes % 64 or not 1 <= k <= 64 or nq < (5 if f32 else 3) or allowed * row_bytes < min_bytes:
        return False
    return -(-nq // 8) * allowed * 100 >= -(-nq // 64) * span * pct


GRID = list(itertools.product((1, 3, 64, 65, 128, 129, 256, 257, 1024), (1, 64, 65, 256, 257), (64, 100, 1536), (F16, F32),
                              ((1000, 1000), (500_000, 1_000_000), (100_000, 1_000_000), (60_000, 1_000_000), (1_000_000, 1_000_000)),
                              (0, 128 * MIB), (0, 50, 100)))


def test_plan_masked_wide_is_its_rule_and_plan_masked_is_unchanged():
    assert _native.MFMA_MIN_BATCH == 65
    said_yes = 0
    for nq, k, dim, dtype, (allowed, span), min_bytes, pct in GRID:
        args = (nq, k, dim, dtype, allowed, span, min_bytes, pct)
        assert _native.plan_masked_wide(*args) == rule_wide(*args), args
        assert _native.plan_masked(*args) == rule_tile(*args), args
        said_yes += rule_wide(*args)
    assert 0 < said_yes < len(GRID)


def test_plan_masked_wide_boundaries():
    plan = lambda nq=1024, k=10, dim=1536, dtype=F16, allowed=500_000, span=1_000_000, min_bytes=128 * MIB, pct=100: _native.plan_masked_wide(  # noqa: E731
        nq, k, dim, dtype, allowed, span, min_bytes, pct)
    full = dict(allowed=1_000_000, span=1_000_000)
    assert not plan(_native.MFMA_MIN_BATCH - 1, **full) and plan(_native.MFMA_MIN_BATCH, **full)
    assert not plan(dtype=F32, **full) and not plan(dtype=F32, pct=0, min_bytes=0, **full)
    assert plan(k=256, **full) and not plan(k=257, **full) and not plan(k=0, **full)
    assert plan(dim=100, **full) and plan(dim=16384, **full) and not plan(dim=16385, **full)
    # pct: 0 = wherever the route serves the shape; 100 = byte parity -- 1024 queries are 128 passes over the allowed rows against four tiles over the span
    assert plan(allowed=1, span=1_000_000, min_bytes=0, pct=0) and plan(allowed=31_250, min_bytes=0) and not plan(allowed=31_249, min_bytes=0)
    # 128 queries: one 128-query tile against 16 passes
    assert plan(128, allowed=62_500, min_bytes=0) and not plan(128, allowed=62_499, min_bytes=0)
    rows = 128 * MIB // (1536 * 2)
    assert not plan(allowed=rows, span=rows + 1) and plan(allowed=rows + 1, span=rows + 1)
    for bad in (dict(dtype=7), dict(allowed=-1), dict(allowed=11, span=10), dict(min_bytes=-1), dict(pct=-1), dict(nq=-1)):
        with pytest.raises(ValueError):
            plan(**bad)


# ---- which words and bits a tile reads
def test_the_bit_a_lane_tests_is_the_row_its_register_holds():
    for row0 in (0, 320, 640, 2560 + 320):  # every row0 is a multiple of 320 from a multiple of 32 (a phase start, a row range of whole tiles)
        word, bit, row = mw.tile_reads_32(row0)
        assert (bit >= 0).all() and (bit < 32).all() and np.array_equal(word * 32 + bit, row)
        assert sorted(np.unique(row).tolist()) == list(range(row0, row0 + 320))  # the 320 rows of the tile, each by 32 lanes x ... registers
        w0, n_words, rel, row = mw.tile_reads_16(row0)
        assert n_words == 3 and (rel >= 0).all() and (rel < 96).all() and np.array_equal(w0 * 32 + rel, row)
        assert set(np.unique(row - w0 * 32 - (rel - rel % 16)).tolist()) <= set(range(16))
        assert sorted(np.unique(row).tolist()) == list(range(row0, row0 + 320))
        # the words a group loads: W .. W + 2 cover its 80 rows exactly, whether it starts at bit 0 or at bit 16
        for wm in range(2):
            for h in range(2):
                g = row0 + 160 * wm + 80 * h
                assert g % 32 in (0, 16) and (g + 79) >> 5 == (g >> 5) + 2


def test_no_word_is_loaded_beyond_the_phase():
    """the 16x16x32 form loads word W + i only while W + i < ceil(r_end / 32), r_end <= rows of the phase: restated for every row tail of the table"""
    for case in mw.CASES:
        begin, end = (0, case.rows) if mw.case_span(case) is None else mw.span_rows(case)
        n_words = -(-(end - begin) // 32)
        for row0 in range(0, end - begin, 320):
            for g in (row0 + 160 * wm + 80 * h for wm in range(2) for h in range(2)):
                if g >= end - begin:
                    continue  # a group behind the row range loads nothing
                loaded = [w for w in range(g >> 5, (g >> 5) + 3) if w < -(-(end - begin) // 32)]
                assert loaded and max(loaded) < n_words and (g >> 5) in loaded


def test_the_table_admits_and_rejects_a_row_at_every_position_of_a_tile():
    admitted = np.zeros(320, dtype=bool)  # row position of a tile (from the span's first row) -> an allowed row there is in some query's masked top k
    rejected = np.zeros(320, dtype=bool)  # ... a disallowed row there is in some query's unmasked top k
    for case in mw.CASES:
        if case.thr != "zero" or mw.case_span(case) is None or case.dups:
            continue
        m = mw.case_mask(case)
        begin, _ = mw.span_rows(case)
        unmasked, masked = mw.oracle_tops(case)
        assert m[masked].all()
        admitted[np.unique((masked - begin) % 320)] = True
        dis = unmasked[~m[unmasked]]
        dis = dis[dis >= begin]
        rejected[np.unique((dis - begin) % 320)] = True
    assert admitted.all() and rejected.all(), (np.flatnonzero(~admitted).tolist(), np.flatnonzero(~rejected).tolist())
    # hence every bit 0 .. 31 and both group offsets (an 80-row group at bit 0 and at bit 16 of its first word)
    assert set((np.flatnonzero(admitted) % 32).tolist()) == set(range(32))


def test_the_table_has_what_the_issue_asks_for():
    by = {c.name: c for c in mw.CASES}
    assert {c.nq for c in mw.CASES} >= {128, 129, 256, 257} and {c.k for c in mw.CASES} >= {1, 10, 64, 65, 256}
    assert {c.thr for c in mw.CASES} == {"zero", "half", "mixed"} and {c.dim for c in mw.CASES} >= {64, 128, 192}
    assert {v for c in mw.CASES for v in c.variants} == {"auto", *mw.VARIANTS}
    assert {c.rows - 320 for c in mw.CASES if c.name.startswith("tail-")} == {79, 80, 81, 159, 160, 161, 319, 320}
    ones = {int(c.mask[4:]) - 320 for c in mw.CASES if c.mask.startswith("one@") and c.mask != "one@last"}
    assert ones == {0, 31, 32, 79, 80, 95, 96, 159, 160, 319}
    assert {c.mask for c in mw.CASES} >= {"all", "alt", "altword", "group80", "group80c", "one@last", "none"}
    assert any(mw.case_garbage(c) and c.rows % 32 for c in mw.CASES)
    g = mw.case_mask(by["mask-group80"])[:320].reshape(4, 80)
    assert g[0].all() and not g[1].any() and g[2].all() and not g[3].any()
    rng = by["mask-range700-1500"]
    assert mw.case_span(rng)[0] % 320 != 0 and mw.span_rows(rng) == (512, 1500)
    # a phase and a row range start mid-mask, every one on a whole word
    assert mw.phase_starts(by["ladder-rand50"]) == [0, 256, 1280] and mw.phase_starts(by["ladder-range300-2600"]) == [256, 512]
    assert mw.range_starts(by["splits-rand50"]) == [0, 960, 1920] and mw.range_starts(by["splits-range700-1900"]) == [512, 1152, 1792]
    for c in (by["ladder-rand50"], by["ladder-range300-2600"]):
        assert all(s % 32 == 0 for s in mw.phase_starts(c))
    # the flagged case: more allowed copies of the query than band_max keys
    f = by["flagged-dups"]
    first, count, qi = f.dups
    assert mw.case_mask(f)[first: first + count].sum() > dict(f.opts)["band_max"] and qi < f.nq


def test_words_are_the_library_bit_form():
    for case in mw.CASES[:6] + [c for c in mw.CASES if mw.case_garbage(c)][:4]:
        m = mw.case_mask(case)
        assert np.array_equal(mw.case_words(case), _native.pack_mask_bits(m))
        bits = np.unpackbits(mw.case_words(case, garbage=True).view(np.uint8), bitorder="little")
        assert np.array_equal(bits[: case.rows].astype(bool), m) and bits[case.rows:].all()


# ---- the ABI
def test_symbols_options_and_defaults():
    lib = _native.load_library(preload_torch=False)
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    for name in ("tavb_search_masked_wide", "tavb_search_masked_wide_device", "tavb_plan_masked_wide"):
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name) and f"int {name}(" in header
    assert _native.ABI_VERSION == 7 and lib.tavb_version() == 7
    for name in ("search_masked_wide", "search_masked_wide_device", "plan_masked_wide", "mask_wide_options"):
        assert hasattr(_native.Engine, name)
    assert '"mask_wide"' in header
