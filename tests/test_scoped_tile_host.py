"""CPU twin of tests/test_gpu_scoped_tile.py: the case table's own claims, the numpy restatement of the membership planes, tavb_plan_scoped,
the five new symbols, and the class' choice between the tile and the row-list route on a recording double."""

from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_tile_cases as st
from tests.test_scoped_batch_host import RecordingEngine, build, pairs
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tavb_search_scoped_tile", "tavb_search_scoped_tile_device", "tavb_search_messages_scoped_tile", "tavb_scope_planes", "tavb_plan_scoped")
F32, F16 = _native.TAVB_F32, _native.TAVB_F16


def test_the_table_is_pinned():
    assert 100 <= len(st.CASES) <= 150
    assert {c.rows for c in st.CASES} == set(st.ROWS) and {c.nq for c in st.CASES} >= set(st.BATCHES) and {c.k for c in st.CASES} == set(st.MAX_HITS)
    assert {(c.family, c.nq) for c in st.CASES if c.group == "family"} == {(f, n) for f in st.FAMILIES for n in st.BATCHES}
    assert {(c.dtype, c.dim, c.rows) for c in st.CASES if c.group == "rows"} == {(dt, d, r) for dt, d in st.SMALL for r in st.ROWS}
    assert {c.thresholds for c in st.CASES} == {"uniform", "per_query"} and any(st.case_garbage(c) for c in st.CASES) and not all(st.case_garbage(c) for c in st.CASES)
    # every instantiation the launcher knows runs somewhere, for both dtypes
    seen = {(c.dtype, r.kernel) for c in st.CASES for r in st.runs(c)}
    from tests import skinny_cases as sc

    assert seen == sc.ALL_KERNELS, sc.ALL_KERNELS - seen
    ladder = [c for c in st.CASES if c.group == "ladder"]
    assert ladder and all(len(sc.phase_bounds(c.rows, 8, 256, 4)) - 1 == 3 for c in ladder)
    assert any(len(c.splits) > 1 for c in st.CASES)


def test_planes_numpy_against_bit_by_bit_construction():
    rng = np.random.default_rng(77)
    for n_masks, rows, first, last in ((1, 40, 0, 39), (31, 300, 5, 280), (33, 700, 300, 650), (65, 257, 0, 256), (97, 1300, 600, 1299)):
        scopes = [rng.random(rows) < 0.4 for _ in range(n_masks)]
        for s in scopes:
            s[:first] = False
            s[last + 1:] = False
        blocks, words, begin = st.plane_shape(n_masks, first, last)
        assert (blocks, words, begin) == _native.scope_plane_shape(n_masks, first, last)
        assert begin % 256 == 0 and begin <= first and words % 32 == 0 and begin + words > last and blocks * 32 >= n_masks
        assert blocks == (1 if n_masks <= 32 else 2 * -(-n_masks // 64))
        want = np.zeros((blocks, words), dtype=np.uint32)
        for b in range(blocks):
            for w in range(words):
                r = begin + w
                for i in range(32):
                    q = 32 * b + i
                    if q < n_masks and r < rows and r <= last and scopes[q][r]:
                        want[b, w] |= np.uint32(1 << i)
        np.testing.assert_array_equal(st.planes_numpy(scopes, first, last), want)
        # the 32 x 32 transpose it is: plane words of a 32-row block, read as a bit matrix, are the masks' words transposed
        packed = np.stack([st.scope_words(s) for s in scopes[:32]])
        blk = (first // 32 + 1) if (first // 32 + 1) * 32 + 31 <= last else first // 32
        bitsq = (packed[:, blk][:, None] >> np.arange(32)[None, :]) & 1  # [query, row]
        got = st.planes_numpy(scopes, first, last)[0, blk * 32 - begin: blk * 32 - begin + 32]
        bitsr = (got[:, None] >> np.arange(32)[None, :]) & 1  # [row, query]
        if blk * 32 >= first and blk * 32 + 31 <= last:
            np.testing.assert_array_equal(bitsr[:, : min(32, n_masks)], bitsq.T[:, : min(32, n_masks)])
    # garbage behind the corpus in a mask's last word is not part of the scope
    assert (st.scope_words(np.ones(33, dtype=bool), garbage=True)[1] == 0xFFFFFFFF) and st.scope_words(np.ones(33, dtype=bool))[1] == 1


MIB = 1 << 20
PLAN = [
    # (nq, k, dim, dtype, gather_rows, span, min_bytes, pct, want, why)
    (64, 10, 1536, F16, 8 * 500_000, 1_000_000, 128 * MIB, 100, True, "64 independent 50 % scopes over 1M x 1536: 1.5 GB per pass, 4M rows against 1M"),
    (64, 10, 1536, F32, 8 * 500_000, 1_000_000, 128 * MIB, 100, True, "the same on fp32"),
    (64, 10, 1536, F16, 8 * 40_000, 1_000_000, 128 * MIB, 100, False, "below the floor: 123 MB per pass"),
    (64, 10, 1536, F16, 8 * 100_000, 1_000_000, 128 * MIB, 100, False, "above the floor, fewer rows than the tile reads"),
    (64, 10, 1536, F16, 8 * 125_000, 1_000_000, 128 * MIB, 100, True, "row parity"),
    (64, 10, 1536, F16, 8 * 125_000, 1_000_000, 128 * MIB, 101, False, "pct tightens"),
    (64, 65, 1536, F16, 8 * 500_000, 1_000_000, 128 * MIB, 100, False, "k > 64"),
    (64, 0, 1536, F16, 8 * 500_000, 1_000_000, 128 * MIB, 100, False, "k < 1"),
    (64, 10, 24, F16, 8 * 500_000, 1_000_000, 0, 0, False, "48-byte rows"),
    (64, 10, 24, F32, 8 * 500_000, 1_000_000, 0, 0, False, "96-byte rows"),
    (2, 10, 1536, F16, 500_000, 500_000, 0, 0, False, "below the tile's own lower bound on fp16 (3)"),
    (4, 10, 1536, F32, 500_000, 500_000, 0, 0, False, "... on fp32 (5)"),
    (64, 10, 32, F16, 1, 1, 0, 0, True, "the probe of scope_tile = 2: yes exactly when the tile serves the shape"),
    (256, 10, 1536, F16, 32 * 500_000, 1_000_000, 128 * MIB, 100, True, "256 queries: 32 passes against 4 tile passes"),
]


@pytest.mark.parametrize("row", PLAN, ids=[r[-1] for r in PLAN])
def test_plan_scoped(row):
    *args, want, _ = row
    assert _native.plan_scoped(*args) is want


def test_plan_scoped_is_monotone_and_checks_its_arguments():
    for dtype in (F16, F32):
        for nq in (8, 33, 64, 200):
            said = [_native.plan_scoped(nq, 10, 1536, dtype, g, 1_000_000) for g in range(0, 30_000_000, 250_000)]
            assert said == sorted(said) and said[0] is False and said[-1] is True, (dtype, nq)
    assert _native.scoped_gather_rows([5, 1, 9, 2, 2, 2, 2, 2, 7, 3]) == 9 + 7 and _native.scoped_gather_rows([]) == 0
    for bad in ((64, 10, 1536, 9, 1, 1), (-1, 10, 1536, F16, 1, 1), (64, 10, 1536, F16, -1, 1), (64, 10, 1536, F16, 1, -1)):
        with pytest.raises(ValueError):
            _native.plan_scoped(*bad)


def test_header_binding_and_library_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    lib = _native.load_library()
    assert lib.tavb_version() == _native.ABI_VERSION == 7 == int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1))
    assert int(re.search(r"#define TAVB_KERNEL_COUNT (\d+)", header).group(1)) == 10
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    for method in ("search_scoped_tile", "search_scoped_tile_device", "search_messages_scoped_tile", "scope_planes", "plan_scoped", "scope_tile_options"):
        assert callable(getattr(_native.Engine, method))
    assert callable(_native.plan_scoped)
    ctx = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_ctx.h")).read()
    body = ctx[ctx.index("void for_each_buffer(F&& f) {"):]
    assert "&d_scope_planes" in body[: body.index("\n  }\n")]
    abi = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_abi.hip")).read()
    assert 'RANGE("scope_tile", scope_tile, 0, 2)' in abi and "int64_t scope_tile = 1;" in ctx
    assert not "scope_tile".startswith(("scan_", "mfma_", "comm_", "topk_", "sort_", "direct_", "small_direct_", "last_"))


def test_the_entry_points_refuse_a_null_context():
    """Without a GPU there is no context, and the context is what every entry point checks first: what this pins is that the new symbols take
    these argument lists, refuse them with a message and write nothing.  The checks behind the context are exercised on the device."""
    lib = _native.load_library()
    q, thr = np.zeros((2, 16), dtype=np.float32), np.zeros(2, dtype=np.float32)
    ords, scs, cnts = np.full((2, 3), 7, dtype=np.int64), np.full((2, 3), 7, dtype=np.float32), np.full(2, 7, dtype=np.int32)
    ptrs = (ctypes.c_void_p * 2)(None, None)
    a = _native._addr
    for k, masks in ((3, ptrs), (0, ptrs), (65, None)):
        assert lib.tavb_search_scoped_tile(None, a(q), 2, masks, 10, 0, 9, k, a(thr), a(ords), a(scs), a(cnts)) == -1 and b"null context" in lib.tavb_last_error()
        assert lib.tavb_search_scoped_tile_device(None, a(q), 2, masks, 10, 0, 9, k, a(thr), a(ords)) == -1 and b"null context" in lib.tavb_last_error()
        assert lib.tavb_search_messages_scoped_tile(None, a(q), 2, masks, 10, 0, 9, k, a(thr), 5, a(ords), a(scs), a(cnts)) == -1
        assert b"null context" in lib.tavb_last_error()
        assert lib.tavb_scope_planes(None, masks, 2, 10, 0, 9, a(ords)) == -1 and b"null context" in lib.tavb_last_error()
    assert ords.min() == 7 and scs.min() == 7 and cnts.min() == 7  # nothing was written


# ---- the class on a recording double ---------------------------------------------------------------------------------------------------------

N, D = 700, 16


class TileEngine(RecordingEngine):
    """RecordingEngine plus the tile calls; `plan` is what plan_scoped answers under scope_tile = 1 (the arguments are recorded)."""

    plan = False

    def __init__(self, device=None, use_torch_stream=False):
        super().__init__(device, use_torch_stream)
        self.options.update({"scope_tile": 1, "mask_tile_min_bytes": 128 << 20, "mask_tile_pct": 100})
        self.plans: list = []

    def plan_scoped(self, nq, k, dim, dtype, gather_rows, span, min_bytes, pct):
        self.plans.append((nq, k, dim, dtype, gather_rows, span, min_bytes, pct))
        return _native.plan_scoped(nq, k, dim, dtype, gather_rows, span, min_bytes, pct) if (min_bytes, pct) == (0, 0) else self.plan

    def search_scoped_tile(self, queries, dev_bits_list, k, thrs, span=None):
        dev_bits_list = list(dev_bits_list)
        assert len(dev_bits_list) == len(queries) and queries.flags.c_contiguous and np.asarray(thrs).shape == (len(queries),)
        self.calls.append(("scoped_tile", [b.data_ptr() for b in dev_bits_list], np.array(queries), span))
        return self._batch(queries, [self._rows_of(b) for b in dev_bits_list], k, thrs)

    def search_messages_scoped_tile(self, queries, dev_bits_list, k, thrs, max_messages, span=None):
        n = len(self.calls)
        out = self.search_messages_scoped(queries, dev_bits_list, k, thrs, max_messages)
        self.calls[n] = ("messages_scoped_tile",) + self.calls[n][1:] + (span,)
        return out


@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 9960)
    return v, make_queries(9, D, 9961), np.random.default_rng(9962).integers(-1, 60, N)


def _masks():
    rng = np.random.default_rng(9963)
    a, b, c = rng.random(N) < 0.5, rng.random(N) < 0.2, np.arange(N) % 3 == 0
    a[:300] = False
    b[:270] = False
    c[:280] = False
    c[650:] = False
    return {"a": a, "b": b, "c": c, "empty": np.zeros(N, dtype=bool)}


def test_the_tile_only_when_option_and_plan_say_so(monkeypatch, corpus):
    v, qs, _ = corpus
    vb = build(monkeypatch, v, TileEngine)
    eng = vb.engine
    masks = _masks()
    h = {name: vb.row_mask(m) for name, m in masks.items()}
    order = ["a", "b", "empty", "a", "c", "b", "a", "empty", "c"]
    thr = [0.0, 0.45, 0.0, 0.5, None, 0.4, 0.55, 0.0, 1.5]
    given = [h[name] for name in order]
    first = min(int(np.flatnonzero(masks[n])[0]) for n in "abc")
    last = max(int(np.flatnonzero(masks[n])[-1]) for n in "abc")

    def routes():
        out = [c[0] for c in eng.calls]
        eng.calls.clear()
        return out

    # scope_tile = 1, the plan says no: the row-list route; the plan saw the searched scopes' counts in submission order and the union's span
    want = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, thr)
    assert routes() == ["scoped"]
    counts = [h[n].count for n in ("a", "a", "a", "b", "b", "c", "c")]
    assert eng.plans == [(7, 7, D, eng.dtype, max(counts), last + 1 - first // 256 * 256, 128 << 20, 100)]
    # ... the plan says yes: the tile, with the same masks in the same order, the span of the union, and the answers scattered back
    eng.plan = True
    got = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, thr)
    (name, ptrs, sent, span), = eng.calls
    assert name == "scoped_tile" and span == (first, last)
    name_of = {h[n].dev_bits.data_ptr(): n for n in masks}
    assert [name_of[p] for p in ptrs] == ["a", "a", "a", "b", "b", "c", "c"]  # equal handles adjacent, groups by first query, no empty scope
    np.testing.assert_array_equal(sent, qs[[0, 3, 6, 1, 5, 4, 8]])
    eng.calls.clear()
    assert [pairs(x) for x in got] == [pairs(x) for x in want] and got[2] == [] and got[7] == [] and got[8] == []
    for i, name in enumerate(order):
        ref = vo.lookup_in_subset(v, qs[i], np.flatnonzero(masks[name]).tolist(), 7, 0.0 if thr[i] is None else thr[i])
        assert [x for x, _ in pairs(got[i])] == [x for x, _ in ref], (i, name)
    o, s, c = vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, thr, as_arrays=True)
    assert routes() == ["scoped_tile"] and c.tolist() == [len(x) for x in got] and all(o[i, : c[i]].tolist() == [x.item for x in got[i]] for i in range(9))
    # scope_tile = 0: never, and the plan is not asked; = 2: wherever the tile serves the shape, whatever the plan of mode 1 says
    eng.plans.clear()
    eng.set_option("scope_tile", 0)
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, thr)
    assert routes() == ["scoped"] and eng.plans == []
    eng.plan = False
    eng.set_option("scope_tile", 2)
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 7, thr)
    assert routes() == ["scoped_tile"] and eng.plans == [(64, 7, D, eng.dtype, 1, 1, 0, 0)]
    # the order of decisions: identical handles go to the one-mask call first; max_hits > 64 keeps the row-list route; raw arrays resolve to handles
    vb.fuzzy_lookup_embeddings_scoped(qs[:5], [h["a"]] * 5, 7)
    assert routes() == ["one_scope"]
    vb.fuzzy_lookup_embeddings_scoped(qs, given, 65, thr)
    assert routes() == ["scoped"]
    vb.fuzzy_lookup_embeddings_scoped(qs[:4], [masks["a"], masks["b"], masks["a"], masks["b"]], 7, 0.0)
    assert routes() == ["scoped_tile"]
    assert vb.fuzzy_lookup_embeddings_scoped(qs[:3], [np.zeros(N, dtype=bool) for _ in range(3)], 7) == [[], [], []] and routes() == []


def test_the_message_form_takes_the_same_decision(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v, TileEngine)
    vb.set_row_messages(rm)
    eng = vb.engine
    masks = _masks()
    h = {name: vb.row_mask(m) for name, m in masks.items()}
    given = [h[n] for n in ("a", "b", "empty", "c")]
    want = vb.lookup_messages_by_embeddings_scoped(qs[:4], given, 7, 0.0)
    assert [c[0] for c in eng.calls if c[0].startswith("messages")] == ["messages_scoped"]
    eng.calls.clear()
    eng.set_option("scope_tile", 2)
    got = vb.lookup_messages_by_embeddings_scoped(qs[:4], given, 7, 0.0)
    calls = [c for c in eng.calls if c[0].startswith("messages")]
    assert [c[0] for c in calls] == ["messages_scoped_tile"] and calls[0][-1] == (min(h[n].span[0] for n in "abc"), max(h[n].span[1] for n in "abc"))
    assert [pairs(x) for x in got] == [pairs(x) for x in want] and got[2] == []
