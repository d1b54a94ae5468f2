"""CPU suite: top-k distinct messages on the 32/64-query tile (engine option "top_messages_tile", tavb_search_top_messages_tile) without
a GPU -- the CPU twin of tests/test_gpu_top_messages_tile.py over the same table, tests/top_messages_tile_cases.py.

  1. the table covers every value of every axis, its generators do what their names say, and its judge accepts the reference's own answer;
  2. at most 10 % of the table's (case, query) pairs are threshold-ambiguous for the reference (the GPU suite checks the count only
     where no message sits at the threshold);
  3. tavb_plan_top_messages_tile as a pure function;
  4. the class on a recording engine double: the tile is called exactly where option and plan allow it, everything else goes as before;
  5. header, option table and binding agree on the new names, and the ABI version stays 7."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import top_messages_tile_cases as tc
from tests.fakes import NullModel
from tests.test_top_messages_scoped_host import RecordingEngine
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tavb_search_top_messages_tile", "tavb_search_top_messages_tile_device", "tavb_plan_top_messages_tile")
F16, F32 = _native.TAVB_F16, _native.TAVB_F32


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_every_axis():
    cases = tc.CASES
    assert 100 <= len(cases) <= 300 and len({c.name for c in cases}) == len(cases)
    assert {c.corpus.rows for c in cases} == set(tc.ROWS) == {1, 31, 32, 33, 255, 256, 257, 513, 2049, 4099}
    assert {c.corpus.dim for c in cases if c.corpus.dtype == "float16"} == set(tc.WIDTHS_F16) == {32, 64, 96, 1536}
    assert {c.corpus.dim for c in cases if c.corpus.dtype == "float32"} == set(tc.WIDTHS_F32) == {16, 32, 48, 384}
    assert {c.nq for c in cases} == set(tc.QUERIES) == {1, 31, 32, 33, 64, 65, 129}
    assert {c.map for c in cases} == set(tc.MAPS)
    assert {c.k for c in cases} == set(tc.KS) == {1, 10, 65, 257, "n", "n+5"}
    assert {c.thresholds for c in cases} == set(tc.THRESHOLDS)
    assert {c.mask for c in cases} == set(tc.MASKS) == {"none", "random50", "range", "ones", "empty"}
    # both K-step sizes and a multi-step loop for either dtype; every row size a multiple of 64 bytes
    for dtype, size in (("float16", 2), ("float32", 4)):
        row_bytes = {c.corpus.dim * size for c in cases if c.corpus.dtype == dtype}
        assert all(b % 64 == 0 for b in row_bytes)
        assert any(b == 64 for b in row_bytes) and any(b == 128 for b in row_bytes) and any(b % 128 and b > 64 for b in row_bytes) and any(b > 256 and b % 128 == 0 for b in row_bytes)
    floor = [c for c in cases if c.scores_bytes]
    assert len(floor) == 1 and floor[0].scores_bytes == 4096 and 1 < tc.group_size(floor[0]) < 64 < floor[0].nq
    assert any(tc.case_k(c) > 64 and c.mask != "empty" and c.thresholds != "above" for c in cases)


def test_the_generators_do_what_they_say():
    for case in tc.CASES:
        rows = case.corpus.rows
        mask = tc.case_mask(case)
        if case.mask == "none":
            assert mask is None
        elif case.mask == "ones":
            assert mask.all()
        elif case.mask == "empty":
            assert not mask.any()
        elif case.mask == "range" and rows >= 256:
            first = int(np.flatnonzero(mask)[0])
            assert first % 32 != 0 and mask[first: int(np.flatnonzero(mask)[-1]) + 1].all() and not mask.all()
        elif case.mask == "random50" and rows >= 255:
            assert 0.4 < mask.mean() < 0.6
        assert tc.expected_kernel(case) in (6432, 6464, 12832, 12864)
    big = next(c for c in tc.CASES if c.corpus.rows == 4099 and c.map == "chunks3")
    rm = tc.message_map(big.corpus.rows, big.map)
    assert rm[31] == rm[32] == 10 and rm[255] == rm[256] == 85  # a message across a 32-row block and across a tile
    v, held, qs = tc.corpus_arrays(big.corpus)
    assert qs.shape == (tc.MAX_QUERIES, big.corpus.dim) and np.isnan(v[big.corpus.rows // 3]).all() and not v[big.corpus.rows // 2].any()
    per = next(c for c in tc.CASES if c.thresholds == "per_query" and c.nq >= 4)
    assert tc.case_thresholds(per)[:4] == [0.0, tc.tenth_threshold(per.corpus), 1.5, 0.5]


# ---- 1. + 2. the judge accepts the reference's own answer; few pairs are threshold-ambiguous ------------------------------------------------

def test_the_judge_accepts_the_reference_and_few_pairs_sit_at_the_threshold():
    pairs = ambiguous = 0
    for case in tc.CASES:
        for qi in range(case.nq):
            items, scores = tc.expected(case, qi)
            rep = tc.judge(case, qi, items, scores)
            assert rep.tie_permuted_positions == 0
            pairs += 1
            ambiguous += rep.threshold_ambiguous > 0
    assert pairs > 3000 and ambiguous <= 0.10 * pairs, (ambiguous, pairs)
    # ... and refuses a wrong one: a score off by more than SCORE_TOL, a swapped pair, a missing message
    case = next(c for c in tc.CASES if c.mask == "none" and c.thresholds == "zero" and c.corpus.rows >= 255 and c.map == "chunks3" and tc.case_k(c) >= 10)
    items, scores = tc.expected(case, 0)
    with pytest.raises(AssertionError):
        tc.judge(case, 0, items, scores + np.float32(3 * vo.SCORE_TOL))
    with pytest.raises(AssertionError):
        tc.judge(case, 0, np.r_[items[1], items[0], items[2:]], np.r_[scores[1], scores[0], scores[2:]])
    with pytest.raises(AssertionError):
        tc.judge(case, 0, items[1:], scores[1:])


# ---- 3. the plan ---------------------------------------------------------------------------------------------------------------------------

def test_the_plan_is_a_pure_function():
    plan = _native.plan_top_messages_tile
    rows = 1_000_000
    # unmasked: the width and the smallest batch decide
    assert [plan(nq, 1536, F32, rows, rows) for nq in (1, 7, 8, 64, 1000)] == [False, False, True, True, True]
    assert plan(8, 1536, F16, rows, rows) and plan(8, 32, F16, rows, rows) and plan(8, 16, F32, rows, rows)
    assert not plan(64, 8, F32, rows, rows) and not plan(64, 24, F16, rows, rows) and not plan(64, 0, F32, rows, rows)  # no K step of the tile
    assert plan(5, 1536, F32, rows, rows, min_batch=5) and not plan(4, 1536, F32, rows, rows, min_batch=5)
    assert plan(1, 1536, F32, 1, 1, 0, 0, 0) and not plan(0, 1536, F32, 1, 1, 0, 0, 0)
    # under a mask: tavb_plan_masked's byte rule -- ceil(nq / 8) x allowed against ceil(nq / 64) x span x pct % -- and its floor
    assert plan(64, 1536, F32, rows // 8, rows) and not plan(64, 1536, F32, rows // 8 - 1, rows)
    assert plan(16, 1536, F32, rows // 2, rows) and not plan(16, 1536, F32, rows // 2 - 1, rows)
    assert plan(16, 1536, F32, rows // 4, rows, pct=50) and not plan(16, 1536, F32, rows // 4 - 1, rows, pct=50)
    assert not plan(64, 1536, F16, 40_000, 40_000 + 1) and plan(64, 1536, F16, 40_000, 40_000 + 1, min_bytes=0)  # 117 MiB of allowed rows
    assert plan(64, 1536, F16, 40_000, 40_000)  # (no floor without a mask: the row scan has none either)
    lib = _native.load_library(preload_torch=False)
    for bad in ((9, 64, 7, 10, 10, 8, 0, 100), (-1, 64, F32, 10, 10, 8, 0, 100), (9, 64, F32, 11, 10, 8, 0, 100), (9, 64, F32, 10, 10, -1, 0, 100)):
        assert lib.tavb_plan_top_messages_tile(*bad) < 0


# ---- 4. the class on a recording double ----------------------------------------------------------------------------------------------------

class TileEngine(RecordingEngine):
    """RecordingEngine with the tile call: the same numpy answer, recorded as ("tile", queries, masked, span)."""

    plan_top_messages_tile = staticmethod(_native.plan_top_messages_tile)

    def __init__(self, device=None, use_torch_stream=False):
        super().__init__(device, use_torch_stream)
        self.options.update(top_messages_tile=0, top_messages_tile_min_batch=_native.TOP_MESSAGES_TILE_MIN_BATCH,
                            mask_tile_min_bytes=_native.MASK_TILE_MIN_BYTES, mask_tile_pct=_native.MASK_TILE_PCT)

    def search_top_messages_tile(self, queries, k, thrs, dev_bits=None, span=None):
        assert 1 <= k <= _native.MAX_LARGE_K and (dev_bits is None) == (span is None)
        self.calls.append(("tile", len(queries), dev_bits is not None, span))
        rows = np.arange(self.rows, dtype=np.int64) if dev_bits is None else self._rows_of(dev_bits)
        if span is not None:
            assert len(rows) and (int(rows[0]), int(rows[-1])) == tuple(span)
        return self._top(queries, [rows] * len(queries), k, thrs)


N, D = 300, 32


@pytest.fixture()
def vb(monkeypatch):
    from tests.synth import make_corpus

    monkeypatch.setattr(_native, "Engine", TileEngine)
    v, _ = make_corpus(N, D, 9960)
    out = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    out.add_embeddings(None, v)
    out.set_row_messages(tc.message_map(N, "chunks3"))
    return out


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def test_the_tile_is_called_exactly_where_option_and_plan_allow(vb):
    from tests.synth import make_queries

    qs = make_queries(20, D, 9961)
    eng = vb.engine
    dense = vb.row_mask(np.arange(N) % 8 != 0)
    sparse = vb.row_mask(np.arange(N) % 16 == 0)
    kinds = lambda: [c[0] for c in eng.calls]  # noqa: E731

    def run(nq, handle=None, k=7, thr=0.0):
        eng.calls.clear()
        got = vb.lookup_top_messages_by_embeddings(qs[:nq], k, thr, handle)
        return kinds(), got

    # the default: never
    assert eng.get_option("top_messages_tile") == 0
    assert run(20)[0] == run(20, dense)[0] == ["one_mask"]
    base = run(20, dense)[1]
    # 2: wherever the tile serves the shape -- any batch, any mask that holds its bits; the span goes along
    eng.set_option("top_messages_tile", 2)
    assert run(1)[0] == run(20)[0] == run(20, dense)[0] == run(3, sparse)[0] == ["tile"]
    assert eng.calls[-1] == ("tile", 3, True, (0, 288))
    assert [bits32(g) for g in run(20, dense)[1]] == [bits32(b) for b in base]
    # ... per-query thresholds pass through, and K outside the native range, K = 0 and an empty mask go as before
    eng.calls.clear()
    thr = [0.0, 0.5, 0.55]
    got = vb.lookup_top_messages_by_embeddings(qs[:3], 7, thr)
    assert kinds() == ["tile"]
    for i in range(3):
        assert bits32(got[i]) == bits32(vb.lookup_top_messages_by_embedding(qs[i], 7, thr[i]))
    assert "tile" not in run(2, k=0)[0] and "tile" not in run(2, k=_native.MAX_LARGE_K + 1)[0]
    assert run(2, vb.row_mask(np.zeros(N, dtype=bool))) == ([], [[], []])
    # 1: the plan -- min_batch for an unmasked batch; under a mask the byte rule and the floor as well
    eng.set_option("top_messages_tile", 1)
    assert run(7)[0] == ["one_mask"] and run(8)[0] == ["tile"]
    assert run(20, dense)[0] == ["one_mask"]  # (300 rows are far below "mask_tile_min_bytes")
    eng.set_option("mask_tile_min_bytes", 0)
    assert run(20, dense)[0] == ["tile"] and run(20, sparse)[0] == ["one_mask"] and run(7, dense)[0] == ["one_mask"]
    eng.set_option("top_messages_tile_min_batch", 1)
    assert run(1)[0] == ["tile"]
    # "top_messages" = 0 wins: the host collapse
    eng.set_option("top_messages", 0)
    assert "tile" not in run(20)[0] and "one_mask" not in kinds()
    eng.set_option("top_messages", 1)
    # a mask without its packed bits (a device group's, a double's) keeps the row list
    eng.set_option("top_messages_tile", 2)
    dense.dev_bits = None
    assert run(20, dense)[0] == ["one_mask"]
    # the adapter inherits the route; the scoped call does not take it
    eng.calls.clear()
    rm = tc.message_map(N, "chunks3")
    adapters.lookup_top_messages(vb, qs[:4], rm, 5)
    adapters.lookup_top_messages(vb, qs[0], rm, 5, scope=[1, 2, 3])
    assert kinds() == ["tile", "tile"]
    eng.calls.clear()
    a, b = vb.row_mask(np.arange(N) % 2 == 0), vb.row_mask(np.arange(N) % 3 == 0)
    vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], 5, 0.0)
    assert kinds() == ["scoped"]


def test_a_width_the_tile_does_not_serve_keeps_the_row_scan(monkeypatch):
    from tests.synth import make_corpus, make_queries

    monkeypatch.setattr(_native, "Engine", TileEngine)
    v, _ = make_corpus(100, 24, 9962)  # 96 bytes per fp32 row: no K step
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb.add_embeddings(None, v)
    vb.set_row_messages(tc.message_map(100, "own"))
    for mode in (1, 2):
        vb.engine.set_option("top_messages_tile", mode)
        vb.engine.calls.clear()
        vb.lookup_top_messages_by_embeddings(make_queries(12, 24, 9963), 5, 0.0)
        assert [c[0] for c in vb.engine.calls] == ["one_mask"]


# ---- 5. header, option table, binding ------------------------------------------------------------------------------------------------------

def test_header_option_table_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    abi = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_abi.hip")).read()
    lib = _native.load_library(preload_torch=False)
    assert lib.tavb_version() == _native.ABI_VERSION == 7 == int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1))
    for name in NEW_SYMBOLS:
        assert name in _native.ABI_SYMBOLS and re.search(rf"\bint {name}\(", header) and getattr(lib, name)
    for option in ("top_messages_tile", "top_messages_tile_min_batch"):
        assert f'"{option}"' in header and f'RANGE("{option}"' in abi
    for method in ("search_top_messages_tile", "search_top_messages_tile_device", "plan_top_messages_tile", "top_messages_tile_options"):
        assert hasattr(_native.Engine, method)
    ctx = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_ctx.h")).read()
    assert re.search(r"int64_t top_messages_tile = 0;", ctx), "the default is 0: no existing call changes its answer"
    assert int(re.search(r"kTopMessagesTileMinBatch = (\d+);", ctx).group(1)) == _native.TOP_MESSAGES_TILE_MIN_BATCH
    assert "10 = a top-messages batch on the" in header
    # a null context is refused with its message, before anything else is read
    assert lib.tavb_search_top_messages_tile(None, None, 1, 5, None, None, 0, 0, 0, None, None, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_top_messages_tile_device(None, None, 1, 5, None, None, 0, 0, 0, None) == -1 and b"null context" in lib.tavb_last_error()
