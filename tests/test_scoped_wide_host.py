"""CPU twin of tests/test_gpu_scoped_wide.py: the case table's own claims, `plane_reads_32` / `plane_reads_16` against what the accumulator
registers hold, tavb_plan_scoped_wide, the four new symbols, and the class' choice between the wide route, the 32/64-query tile and the row
list on a recording double."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from tests import scoped_batch_cases as sb
from tests import scoped_wide_cases as sw
from tests.test_scoped_batch_host import RecordingEngine, build, pairs
from tests.test_scoped_tile_host import TileEngine, _masks
from tests.synth import make_corpus, make_queries
from tests.wide256_cases import TILE_ROWS
from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tavb_search_scoped_wide", "tavb_search_scoped_wide_device", "tavb_search_messages_scoped_wide", "tavb_plan_scoped_wide")
F32, F16 = _native.TAVB_F32, _native.TAVB_F16


def test_the_table_is_pinned():
    cases = sw.CASES
    assert 40 <= len(cases) <= 60 and len(sw.RUNS) <= 160
    assert {c.nq for c in cases} >= {128, 129, 256, 257} and {c.k for c in cases} == {1, 10, 64, 65, 256}
    assert {c.dim for c in cases} == {64, 128, 192, 100} and all(TILE_ROWS + 79 <= c.rows <= 2600 for c in cases)
    assert {c.thr for c in cases} == {"zero", "half", "mixed"}
    thr = sw.case_thresholds(next(c for c in cases if c.thr == "mixed"))
    assert np.isnan(thr).any() and (thr > 1).any() and (thr == 0).any()
    # every family of the scoped batches at least once on each of the four variants, and this table's own
    for fam in sb.FAMILIES:
        assert {v for c in cases if c.family == fam for v in c.variants} == set(sw.ALL_VARIANTS), fam
    for fam in sw.OWN_FAMILIES:
        assert {v for c in cases if c.family == fam for v in c.variants} == set(sw.ALL_VARIANTS), fam
    assert {c.rows - TILE_ROWS for c in cases if c.name.startswith("tail-")} == set(sw.ROW_TAILS)
    assert all(sw.case_garbage(c) for c in cases if c.name.startswith("tail-")) and not all(sw.case_garbage(c) for c in cases)
    assert set(sw.VARIANTS) == {"t128", "t256m16", "t256m32", "t256bd"} and dict(sw.ROUTE_OPTS) == {"scope_wide": 2, "scope_tile": 0}


def test_the_scope_families_do_what_the_table_says():
    by = {c.name: c for c in sw.CASES}
    # mod32 / mod16: the scopes of the queries of one 32-block (16-fragment) all differ; a query's rows sit at one bit of every mask word
    for name, m in (("mod32", 32), ("mod16", 16)):
        scopes = sw.case_scopes(by[name])
        for q in (0, 1, m - 1, m, 255):
            assert np.flatnonzero(scopes[q]).tolist() == list(range(q % m, by[name].rows, m))
        assert len({s.tobytes() for s in scopes[:m]}) == m
    # single / single7: one row each, and every row position of the second tile is some query's
    for name in ("single", "single7"):
        scopes = sw.case_scopes(by[name])
        only = [np.flatnonzero(s) for s in scopes]
        assert all(len(o) == 1 for o in only) and sorted(int(o[0]) for o in only) == list(range(TILE_ROWS, 2 * TILE_ROWS))
    assert [int(np.flatnonzero(s)[0]) - TILE_ROWS for s in sw.case_scopes(by["single7"])[:4]] == [0, 7, 14, 21]
    # the ladder case: two phases, the span begins mid-corpus, and some queries have no allowed row in the first
    lad = by["ladder-disjoint"]
    scopes = sw.case_scopes(lad)
    first, last = sw.union_span(scopes)
    assert (first, last) == (300, 2599) and first // 256 * 256 == 256
    from tests.wide256_cases import ladder_bounds

    o = dict(lad.opts)
    bounds = ladder_bounds(last + 1 - 256, o["mfma_sample_rows"], o["mfma_ladder"])
    assert len(bounds) - 1 >= 2 and bounds[1] == 256
    in_first = [bool(s[256: 256 + bounds[1]].any()) for s in scopes]
    assert not all(in_first) and any(in_first) and in_first[:44] == [False] * 44
    # the flagged cases: more ties at the query's best score than band_max keys, every other copy in its scope
    for name in ("flagged-dups", "waves-flagged"):
        c = by[name]
        lo, count, qi = c.dups
        v, _, qs = sw.case_inputs(c)
        scope = sw.case_scopes(c)[qi]
        assert scope[lo: lo + count].sum() == count // 2 > dict(c.opts)["band_max"] and not scope[lo + 1]
        assert (v[lo: lo + count] == v[lo]).all()
    wf = by["waves-flagged"]
    assert all(wf.dups[2] >= sw.variant_tile(v) for v in wf.variants)  # the flagged query is not in the first wave
    assert sw.waves(by["waves-random50%"], "t128") == 5 and sw.waves(by["waves-random50%"], "t256m16") == 3 and sw.waves(by["k10"], "t128") == 1
    # garbage only behind the corpus
    s = np.zeros(33, dtype=bool)
    assert sw.scope_words(s, garbage=True).tolist() == [0, 0xFFFFFFFE] and sw.scope_words(s).tolist() == [0, 0]


@pytest.mark.parametrize("tile", [128, 256])
def test_plane_reads_32_name_the_row_and_query_each_register_holds(tile):
    for row0, qtile in ((0, 0), (TILE_ROWS, 1), (7 * TILE_ROWS, 3)):
        block, word, bit = sw.plane_reads_32(row0, qtile, tile)
        row, query = sw.acc_holds_32(row0, qtile, tile)
        np.testing.assert_array_equal(word, row)
        np.testing.assert_array_equal(32 * block + bit, query)
        # every (row, query) of the tile exactly once: all 320 row positions, all `tile` query positions
        flat = (row - row0).ravel() * tile + (query - qtile * tile).ravel()
        assert np.array_equal(np.sort(flat), np.arange(TILE_ROWS * tile))
        # a block's 32 words are whole planes' words: they start at a multiple of 32 rows and stay inside one plane block
        first = word.min(axis=(4, 5))
        assert (first % 32 == 0).all() and ((word - first[..., None, None]) < 32).all() and (block == block[..., :1, :1]).all()


def test_plane_reads_16_name_the_row_and_query_each_register_holds():
    for row0, qtile in ((0, 0), (TILE_ROWS, 1), (7 * TILE_ROWS, 3)):
        block, word, bit = sw.plane_reads_16(row0, qtile)
        row, query = sw.acc_holds_16(row0, qtile)
        np.testing.assert_array_equal(word, row)
        np.testing.assert_array_equal(32 * block + bit, query)
        flat = (row - row0).ravel() * 256 + (query - qtile * 256).ravel()
        assert np.array_equal(np.sort(flat), np.arange(TILE_ROWS * 256))
        # per (group, fragment, m) the 16 words of one load: from a multiple of 16 rows on, one plane block, one 16-bit half
        first = word.min(axis=(4, 6))  # over lanes and j
        assert (first % 16 == 0).all()
        assert ((word - first[:, :, :, :, None, :, None]) < 16).all()
        assert ((bit >> 4) == (bit >> 4)[:, :, :, :, :1, :1, :1]).all() and (block == block[:, :, :, :, :1, :1, :1]).all()


MIB = 1 << 20
PLAN = [
    # (nq, k, dim, dtype, gather_rows, span, min_bytes, pct, want, why)
    (128, 10, 1536, F16, 16 * 500_000, 1_000_000, 128 * MIB, 100, True, "128 independent 50 % scopes over 1M x 1536: 8M rows against one pass of 1M"),
    (128, 10, 1536, F32, 16 * 500_000, 1_000_000, 128 * MIB, 100, False, "fp32: not built"),
    (64, 10, 1536, F16, 8 * 500_000, 1_000_000, 128 * MIB, 100, False, "below the wide tile's lower bound (65)"),
    (65, 10, 1536, F16, 9 * 500_000, 1_000_000, 128 * MIB, 100, True, "at the bound"),
    (128, 257, 1536, F16, 16 * 500_000, 1_000_000, 128 * MIB, 100, False, "k = 257"),
    (128, 0, 1536, F16, 16 * 500_000, 1_000_000, 128 * MIB, 100, False, "k < 1"),
    (128, 256, 1536, F16, 32 * 500_000, 1_000_000, 128 * MIB, 100, True, "k = 256: 32 passes of four"),
    (128, 10, 1536, F16, 16 * 40_000, 1_000_000, 128 * MIB, 100, False, "below the floor per pass of eight: 123 MB"),
    (128, 10, 1536, F16, 16 * 50_000, 1_000_000, 128 * MIB, 100, False, "above the floor, fewer rows than the tile reads (0.8M against 1M)"),
    (128, 10, 1536, F16, 16 * 62_500, 1_000_000, 128 * MIB, 100, True, "row parity"),
    (128, 10, 1536, F16, 16 * 62_500, 1_000_000, 128 * MIB, 101, False, "pct tightens"),
    (128, 65, 1536, F16, 16 * 62_500, 1_000_000, 128 * MIB, 100, False, "k > 64: the floor counts 32 passes of four"),
    (128, 65, 1536, F16, 32 * 62_500, 1_000_000, 128 * MIB, 100, True, "... which a gather_rows over passes of four meets"),
    (1024, 10, 1536, F16, 128 * 40_000, 1_000_000, 128 * MIB, 100, False, "1024 queries: the floor is per pass whatever the batch"),
    (1024, 10, 1536, F16, 128 * 50_000, 1_000_000, 128 * MIB, 100, True, "1024 queries: 6.4M rows against four passes of 1M"),
    (128, 10, 100, F16, 1, 1, 0, 0, True, "an odd width is served (the zero-padded copy); the probe of scope_wide = 2"),
    (128, 10, 16385, F16, 1, 1, 0, 0, False, "wider than the tile serves"),
]


@pytest.mark.parametrize("row", PLAN, ids=[r[-1] for r in PLAN])
def test_plan_scoped_wide(row):
    *args, want, _ = row
    assert _native.plan_scoped_wide(*args) is want


def test_plan_scoped_wide_on_a_grid_restated():
    """the rule as the header states it, restated: the query tile from tavb_plan_masked_wide's own choice (its answer flips where one more
    tile pass tips the balance), monotone in gather_rows, and the argument checks"""
    def tile_of(nq, span):
        n128 = -(-nq // 128)
        qt = 128 if (n128 & 1 and n128 <= 5) else 256
        if qt == 256 and -(-nq // 256) * -(-span // 320) <= 4 * 256:
            qt = 128
        return qt

    for nq in (65, 128, 129, 256, 257, 640, 1024):
        for k in (10, 64, 65, 256):
            for span in (1_000, 100_000, 1_000_000):
                for gather in (0, span // 2, span, 3 * span, 40 * span):
                    for min_bytes in (0, 128 * MIB):
                        per = 4 if k > 64 else 8
                        want = (gather * 1536 * 2 >= -(-nq // per) * min_bytes) and gather * 100 >= -(-nq // tile_of(nq, span)) * span * 100
                        assert _native.plan_scoped_wide(nq, k, 1536, F16, gather, span, min_bytes, 100) is want, (nq, k, span, gather, min_bytes)
                        assert _native.plan_scoped_wide(nq, k, 1536, F32, gather, span, min_bytes, 100) is False
    for nq in (65, 200, 1024):
        said = [_native.plan_scoped_wide(nq, 10, 1536, F16, g, 1_000_000) for g in range(0, 30_000_000, 250_000)]
        assert said == sorted(said) and said[0] is False and said[-1] is True, nq
    for bad in ((128, 10, 1536, 9, 1, 1), (-1, 10, 1536, F16, 1, 1), (128, 10, 1536, F16, -1, 1), (128, 10, 1536, F16, 1, -1)):
        with pytest.raises(ValueError):
            _native.plan_scoped_wide(*bad)
    assert _native.scoped_gather_rows([5, 1, 9, 2, 2, 2, 2, 2, 7, 3], 4) == 9 + 2 + 7


def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    lib = _native.load_library()
    assert lib.tavb_version() == _native.ABI_VERSION == int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1))
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    for method in ("search_scoped_wide", "search_scoped_wide_device", "search_messages_scoped_wide", "plan_scoped_wide", "scope_wide_options"):
        assert callable(getattr(_native.Engine, method))
    ctx = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_ctx.h")).read()
    abi = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_abi.hip")).read()
    assert 'RANGE("scope_wide", scope_wide, 0, 2)' in abi and 'RANGE("scope_wave_bytes", scope_wave_bytes, 1,' in abi
    assert re.search(r"int64_t scope_wide = [01];", ctx) and '"scope_wide"' in header and '"scope_wave_bytes"' in header


def test_the_entry_points_refuse_a_null_context():
    lib = _native.load_library()
    q, thr = np.zeros((2, 16), dtype=np.float32), np.zeros(2, dtype=np.float32)
    ords, scs, cnts = np.full((2, 3), 7, dtype=np.int64), np.full((2, 3), 7, dtype=np.float32), np.full(2, 7, dtype=np.int32)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    a = _native._addr
    for k, masks in ((3, ptrs), (0, ptrs), (257, None)):
        assert lib.tavb_search_scoped_wide(None, a(q), 2, masks, 10, 0, 9, k, a(thr), a(ords), a(scs), a(cnts)) == -1 and b"null context" in lib.tavb_last_error()
        assert lib.tavb_search_scoped_wide_device(None, a(q), 2, masks, 10, 0, 9, k, a(thr), a(ords)) == -1 and b"null context" in lib.tavb_last_error()
        assert lib.tavb_search_messages_scoped_wide(None, a(q), 2, masks, 10, 0, 9, k, a(thr), 5, a(ords), a(scs), a(cnts)) == -1
        assert b"null context" in lib.tavb_last_error()
    assert ords.min() == 7 and scs.min() == 7 and cnts.min() == 7  # nothing was written


# ---- the class on a recording double ---------------------------------------------------------------------------------------------------------

N, D = 700, 16


class WideEngine(TileEngine):
    """TileEngine plus the wide calls; `plan_wide` is what plan_scoped_wide answers under scope_wide = 1 (the arguments are recorded)."""

    plan_wide = False

    def __init__(self, device=None, use_torch_stream=False):
        super().__init__(device, use_torch_stream)
        self.options["scope_wide"] = 1
        self.wide_plans: list = []

    def plan_scoped_wide(self, nq, k, dim, dtype, gather_rows, span, min_bytes, pct):
        self.wide_plans.append((nq, k, dim, dtype, gather_rows, span, min_bytes, pct))
        return True if (min_bytes, pct) == (0, 0) else self.plan_wide

    def search_scoped_wide(self, queries, dev_bits_list, k, thrs, span=None):
        dev_bits_list = list(dev_bits_list)
        assert len(dev_bits_list) == len(queries) and queries.flags.c_contiguous and np.asarray(thrs).shape == (len(queries),)
        self.calls.append(("scoped_wide", [b.data_ptr() for b in dev_bits_list], np.array(queries), span))
        return self._batch(queries, [self._rows_of(b) for b in dev_bits_list], k, thrs)

    def search_messages_scoped_wide(self, queries, dev_bits_list, k, thrs, max_messages, span=None):
        n = len(self.calls)
        out = self.search_messages_scoped(queries, dev_bits_list, k, thrs, max_messages)
        self.calls[n] = ("messages_scoped_wide",) + self.calls[n][1:] + (span,)
        return out


@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 9970)
    return v, make_queries(9, D, 9971), np.random.default_rng(9972).integers(-1, 60, N)


ORDER = ["a", "b", "empty", "a", "c", "b", "a", "empty", "c"]
THR = [0.0, 0.45, 0.0, 0.5, None, 0.4, 0.55, 0.0, 1.5]


def _routes(eng):
    out = [c[0] for c in eng.calls]
    eng.calls.clear()
    return out


def test_the_wide_route_first_when_option_and_plan_say_so(monkeypatch, corpus):
    v, qs, _ = corpus
    vb = build(monkeypatch, v, WideEngine)
    eng = vb.engine
    masks = _masks()
    h = {name: vb.row_mask(m) for name, m in masks.items()}
    given = [h[name] for name in ORDER]
    first = min(int(np.flatnonzero(masks[n])[0]) for n in "abc")
    last = max(int(np.flatnonzero(masks[n])[-1]) for n in "abc")
    counts = [h[n].count for n in ("a", "a", "a", "b", "b", "c", "c")]
    # scope_wide = 1, both plans say no: the row list; the wide plan saw the searched scopes' counts (passes of eight) and the union's span
    want = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, THR)
    assert _routes(eng) == ["scoped"]
    assert eng.wide_plans == [(7, 7, D, eng.dtype, max(counts), last + 1 - first // 256 * 256, 128 << 20, 100)]
    # the wide plan says no, the tile's says yes: the 32/64-query tile, as before
    eng.plan = True
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, THR)
    assert _routes(eng) == ["scoped_tile"]
    # both say yes: the wide route wins, and the tile's plan is not asked; same masks, same order, the union's span, answers scattered back
    eng.plan_wide = True
    eng.plans.clear()
    got = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, THR)
    (name, ptrs, sent, span), = eng.calls
    assert name == "scoped_wide" and span == (first, last) and eng.plans == []
    name_of = {h[n].dev_bits.data_ptr(): n for n in masks}
    assert [name_of[p] for p in ptrs] == ["a", "a", "a", "b", "b", "c", "c"]
    np.testing.assert_array_equal(sent, qs[[0, 3, 6, 1, 5, 4, 8]])
    eng.calls.clear()
    assert [pairs(x) for x in got] == [pairs(x) for x in want] and got[2] == [] and got[7] == [] and got[8] == []
    o, s, c = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, THR, as_arrays=True)
    assert _routes(eng) == ["scoped_wide"] and c.tolist() == [len(x) for x in got]
    # max_hits 65 .. 256: the wide route serves them (the tile does not), with a gather over passes of FOUR
    eng.wide_plans.clear()
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 65, THR)
    assert _routes(eng) == ["scoped_wide"]
    assert eng.wide_plans[0][4] == max(counts[:4]) + max(counts[4:]) and eng.wide_plans[0][1] == 65
    eng.plan_wide = False
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 65, THR)
    assert _routes(eng) == ["scoped"]
    # scope_wide = 0: never, its plan is not asked; = 2: wherever served, whatever the plan of mode 1 says
    eng.wide_plans.clear()
    eng.set_option("scope_wide", 0)
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, THR)
    assert _routes(eng) == ["scoped_tile"] and eng.wide_plans == []
    eng.set_option("scope_wide", 2)
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 256, THR)
    assert _routes(eng) == ["scoped_wide"] and eng.wide_plans == [(128, 256, D, eng.dtype, 1, 1, 0, 0)]
    # unchanged: identical handles go to the one-mask call, empty scopes take no slot, max_hits > 256 and 0 loop
    vb.fuzzy_lookup_embeddings_scoped(qs[:5], [h["a"]] * 5, 7)
    assert _routes(eng) == ["one_scope"]
    assert vb.fuzzy_lookup_embeddings_scoped(qs[:3], [np.zeros(N, dtype=bool) for _ in range(3)], 7) == [[], [], []] and _routes(eng) == []
    for k in (0, 257):
        vb.fuzzy_lookup_embeddings_scoped(qs[:4], given[:4], k, 0.0)
        assert not {"scoped_wide", "scoped_tile", "scoped"} & set(_routes(eng)), k


def test_a_double_without_the_wide_call_keeps_its_route(monkeypatch, corpus):
    v, qs, _ = corpus
    masks = _masks()
    for cls, plan, want in ((RecordingEngine, None, "scoped"), (TileEngine, False, "scoped"), (TileEngine, True, "scoped_tile")):
        vb = build(monkeypatch, v, cls)
        eng = vb.engine
        assert not hasattr(eng, "search_scoped_wide") and not hasattr(eng, "plan_scoped_wide")
        if plan is not None:
            eng.plan = plan
        h = {name: vb.row_mask(m) for name, m in masks.items()}
        vb.fuzzy_lookup_embeddings_scoped(qs, [h[n] for n in ORDER], 7, THR)
        assert _routes(eng) == [want], cls.__name__


def test_the_message_form_takes_the_same_decision(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v, WideEngine)
    vb.set_row_messages(rm)
    eng = vb.engine
    masks = _masks()
    h = {name: vb.row_mask(m) for name, m in masks.items()}
    given = [h[n] for n in ("a", "b", "empty", "c")]
    want = vb.lookup_messages_by_embeddings_scoped(qs[:4], given, 7, 0.0)
    assert [c[0] for c in eng.calls if c[0].startswith("messages")] == ["messages_scoped"]
    eng.calls.clear()
    eng.plan_wide = True
    got = vb.lookup_messages_by_embeddings_scoped(qs[:4], given, 7, 0.0)
    calls = [c for c in eng.calls if c[0].startswith("messages")]
    assert [c[0] for c in calls] == ["messages_scoped_wide"] and calls[0][-1] == (min(h[n].span[0] for n in "abc"), max(h[n].span[1] for n in "abc"))
    assert [pairs(x) for x in got] == [pairs(x) for x in want] and got[2] == []
