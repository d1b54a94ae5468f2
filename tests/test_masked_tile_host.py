"""CPU suite for the masked 32/64-query tile route: the claims of its case table (tests/masked_tile_cases.py) from the float64 oracle alone,
`tavb_plan_masked` at its boundaries, the new symbols and option names, and the routing of `VectorBase.fuzzy_lookup_embeddings_masked` between
the gather route and the tile with an engine double that records its calls."""

import numpy as np
import pytest

from tests import masked_tile_cases as mc
from tests import skinny_cases as sc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

F16, F32 = _native.TAVB_F16, _native.TAVB_F32
MIB = 1 << 20


# ---- the table's own claims
def test_the_table_has_what_the_route_needs():
    by = lambda g: [c for c in mc.CASES if c.group == g]  # noqa: E731
    assert {(c.dtype, c.dim) for c in by("width")} == {("fp16", 64), ("fp16", 96), ("fp16", 1536), ("fp32", 64), ("fp32", 48), ("fp32", 1536)}
    assert sc.k_steps(sc.Case("x", "x", "fp16", 1, 64)) == 1 and sc.step_bytes(96, False) == 64 and sc.step_bytes(48, True) == 64
    assert {c.rows for c in by("rows")} == {1, 31, 32, 33, 255, 256, 257, 600, 1300} and {c.dtype for c in by("rows")} == {"fp16", "fp32"}
    assert {c.mask for c in by("mask")} >= {"all", "none", "one@0", "one@255", "one@256", "one@last", "alt", "wordclear", "wordkeep", "rand50", "rand2", "range300-700"}
    assert {c.nq for c in mc.CASES} == {64, 65} and {c.k for c in mc.CASES} == {64, 10} and {c.thr for c in mc.CASES} == {"zero", "half", "mixed"}
    assert any(c.name.endswith("tailones") and c.rows % 32 and mc.case_garbage(c) for c in mc.CASES)
    for c in mc.CASES:  # every case runs on the 32- and the 64-query tile; whole-line widths on all four other variants as well
        kernels = {r.kernel for r in mc.runs(c)}
        assert {sc.kernel_id(c.dim, c.f32, 32), sc.kernel_id(c.dim, c.f32, 64)} <= kernels, c.name
        if sc.line_steps(c.dim, c.f32):
            assert {22832, 32832, 6432} <= kernels, c.name
    assert any(r.kernel == 52832 for c in mc.CASES for r in mc.runs(c))  # register staging: K steps a multiple of 4 (1536-wide rows)
    assert {r.kernel for c in mc.CASES for r in mc.runs(c)} == {kid for _, kid in sc.ALL_KERNELS}


def test_word_masks_clear_one_word_of_every_wave():
    case = next(c for c in mc.CASES if c.mask == "wordclear")
    m = mc.case_mask(case)[:256].reshape(4, 2, 32)  # [wave, word of the wave, row]
    assert (m.all(axis=2) | ~m.any(axis=2)).all() and ((~m.any(axis=2)).sum(axis=1) == 1).all()
    keep = mc.case_mask(next(c for c in mc.CASES if c.mask == "wordkeep" and c.dtype == case.dtype))
    assert (keep != mc.case_mask(case)).all()
    half = mc.case_mask(case)[:128].reshape(4, 32)  # half tiles: a wave owns one word
    assert (~half.any(axis=1)).sum() == 2


def test_words_are_the_library_bit_form():
    for case in mc.CASES[:8] + [c for c in mc.CASES if c.name.endswith("tailones")]:
        m = mc.case_mask(case)
        assert np.array_equal(mc.case_words(case), _native.pack_mask_bits(m))
        g = mc.case_words(case, garbage=True)
        bits = np.unpackbits(g.view(np.uint8), bitorder="little")
        assert np.array_equal(bits[: case.rows].astype(bool), m) and bits[case.rows:].all()


def test_splits_and_ladder_cases_do_what_they_say():
    for c in (c for c in mc.CASES if c.group == "splits"):
        assert mc.span_rows(c)[1] - mc.span_rows(c)[0] > 5 * 256 and dict(c.opts)["mfma_sample_rows"] == -1
        if 1 in c.splits:  # one workgroup, six tiles: at threshold 0 the allowed rows of the first three leave a buffer above its compaction limit
            assert mc.case_mask(c)[:768].sum() > sc.CAP - sc.TILE_ROWS
        if 8 in c.splits:
            ranges = sc.row_ranges(c.rows, 8)
            assert any(b >= e for b, e in ranges)
    starts = {c.name: mc.case_phase_starts(c) for c in mc.CASES if c.group == "ladder"}
    assert {tuple(s) for s in starts.values()} == {(0, 256, 1280), (256, 512)}, starts
    for c in (c for c in mc.CASES if c.group == "ladder" and c.span == "whole"):  # the first two phases hold no allowed row
        assert not mc.case_mask(c)[:1280].any() and mc.case_span(c) == (0, c.rows - 1)
    for c in mc.CASES:  # every phase starts on a whole word
        if mc.case_span(c) is not None:
            for sp in {*c.splits, 1, 8}:
                assert all(s % 32 == 0 for s in mc.case_phase_starts(c, sp or 1)), c.name
    assert any(mc.span_rows(c)[0] > 0 for c in mc.CASES if mc.case_span(c) is not None)


def test_a_kernel_that_ignores_the_mask_fails_every_query_and_every_word_position_is_seen():
    admitted = np.zeros(8, dtype=bool)  # word position of a 256-row tile -> an allowed row there is in some query's masked top k
    rejected = np.zeros(8, dtype=bool)  # ... a disallowed row there is in some query's unmasked top k
    for case in mc.CASES:
        if case.thr != "zero" or not mc.partial(case):
            continue
        m = mc.case_mask(case)
        unmasked, masked = mc.oracle_tops(case)
        disallowed_in_top = ~m[unmasked]
        assert disallowed_in_top.any(axis=1).all(), f"{case.name}: queries {np.flatnonzero(~disallowed_in_top.any(axis=1)).tolist()} never meet the mask"
        assert m[masked].all()
        admitted[np.unique((masked % 256) // 32)] = True
        rejected[np.unique((unmasked[disallowed_in_top] % 256) // 32)] = True
    assert admitted.all() and rejected.all(), (admitted, rejected)


# ---- tavb_plan_masked
def plan(nq, k=10, dim=1536, dtype=F16, allowed=500_000, span=1_000_000, min_bytes=128 * MIB, pct=100):
    return _native.plan_masked(nq, k, dim, dtype, allowed, span, min_bytes, pct)


def test_plan_masked_support_and_batch_bounds():
    assert plan(32) and plan(64, dtype=F32)
    full = dict(allowed=1_000_000, span=1_000_000)
    assert not plan(2, **full) and plan(3, **full)  # skinny_min_batch_f16 = 3
    assert not plan(4, dtype=F32, **full) and plan(5, dtype=F32, **full)  # skinny_min_batch_f32 = 5
    assert plan(32, k=64) and not plan(32, k=65) and plan(32, k=1) and not plan(32, k=0)
    w = dict(min_bytes=0)  # rows of a multiple of 64 bytes
    assert not plan(32, dim=40, **w) and plan(32, dim=32, **w) and not plan(32, dim=8, dtype=F32, **w) and plan(32, dim=16, dtype=F32, **w)
    for bad in (dict(dtype=7), dict(allowed=-1), dict(allowed=11, span=10), dict(min_bytes=-1), dict(pct=-1), dict(nq=-1)):
        with pytest.raises(ValueError):  # (TAVB_E_INVALID)
            plan(**{"nq": 32, **bad})


def test_plan_masked_min_bytes():
    rows = 128 * MIB // (1536 * 2)  # 43690.67: 43691 fp16 rows are the first to reach 128 MiB
    assert not plan(32, allowed=rows, span=rows + 1) and plan(32, allowed=rows + 1, span=rows + 1)
    assert plan(32, allowed=1, span=1, min_bytes=0) and plan(32, allowed=1, span=1, min_bytes=3072) and not plan(32, allowed=1, span=1, min_bytes=3073)
    assert plan(32, dtype=F32, allowed=rows // 2 + 1, span=rows)  # fp32 rows are twice the bytes


def test_plan_masked_byte_parity():
    # gather = ceil(nq / 8) x allowed, tile = ceil(nq / 64) x span: the tile from gather >= tile
    span = 1_000_000
    for nq, passes, tiles in ((3, 1, 1), (8, 1, 1), (9, 2, 1), (64, 8, 1), (65, 9, 2)):
        edge = -(-tiles * span // passes)  # the fewest allowed rows at parity
        assert plan(nq, allowed=edge, span=span, min_bytes=0), nq
        assert not plan(nq, allowed=edge - 1, span=span, min_bytes=0), nq
    assert not plan(1, allowed=span, span=span, min_bytes=0)  # below the tile's own lower bound whatever the bytes
    # a contiguous range: span == allowed is parity at any batch; the same rows scattered over a span 20 times their number are not
    assert plan(8, allowed=50_000, span=50_000, min_bytes=0) and plan(64, allowed=50_000, span=50_000)
    assert not plan(64, allowed=50_000, span=1_000_000) and not plan(1024, allowed=50_000, span=1_000_000)
    # pct: 50 = the tile already when the gather moves half the tile's bytes; 0 = whenever supported
    assert plan(8, allowed=500_000, span=span, pct=50) and not plan(8, allowed=499_999, span=span, pct=50)
    assert plan(3, allowed=1, span=span, min_bytes=0, pct=0)


def test_symbols_options_and_defaults():
    for name in ("tavb_search_masked_batch", "tavb_search_masked_device", "tavb_plan_masked"):
        assert name in _native.ABI_SYMBOLS and hasattr(_native.load_library(preload_torch=False), name)
    assert _native.ABI_VERSION == 7
    for name in ("search_masked_batch", "search_masked_device", "plan_masked", "mask_to_rows_bits"):
        assert hasattr(_native.Engine, name)
    assert _native.MASK_TILE_MIN_BYTES == 128 * MIB and _native.MASK_TILE_PCT == 100
    header = open(_native.__file__.replace("typeagent_py_amd/_native.py", "include/tavb.h")).read()
    for opt in ("mask_tile", "mask_tile_min_bytes", "mask_tile_pct", "masked_route"):
        assert f'"{opt}"' in header
        assert not opt.startswith(("scan_", "mfma_", "comm_", "topk_", "sort_", "direct_", "small_direct_", "last_"))


# ---- VectorBase routing, with an engine double that records its calls
N, D = 700, 32


class MaskedFake(FakeEngine):
    """FakeEngine + the single-GPU masked calls: numpy arrays stand in for device memory; both routes answer with the oracle's arithmetic"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.calls: list = []
        self.options.update(mask_tile=1, mask_tile_min_bytes=_native.MASK_TILE_MIN_BYTES, mask_tile_pct=_native.MASK_TILE_PCT)

    plan_masked = staticmethod(_native.plan_masked)

    def mask_to_rows_bits(self, mask):
        m = np.asarray(mask)
        flat = np.flatnonzero(m).astype(np.int32)
        return flat, len(flat), _native.pack_mask_bits(m)

    def mask_to_rows(self, mask):
        return self.mask_to_rows_bits(mask)[:2]

    def _subset_batch(self, queries, rows, k, thrs):
        t = np.broadcast_to(np.asarray(thrs, dtype=np.float32), (len(queries),))
        ords, scs, cnts = np.zeros((len(queries), k), np.int64), np.zeros((len(queries), k), np.float32), np.zeros(len(queries), np.int32)
        for i, q in enumerate(queries):
            pos, s = self.search_subset(q, rows, k, t[i])
            ords[i, : len(pos)], scs[i, : len(pos)], cnts[i] = rows[pos] + self.ordinal_base, s, len(pos)
        return ords, scs, cnts

    def search_subset_batch_resident(self, queries, dev_rows, k, thrs, remap=True):
        self.calls.append(("gather", len(queries), k))
        return self._subset_batch(queries, dev_rows.astype(np.int64), k, thrs)

    def search_masked_batch(self, queries, dev_bits, k, thrs, span=None):
        self.calls.append(("tile", len(queries), k, span))
        allowed = np.flatnonzero(np.unpackbits(dev_bits.view(np.uint8), bitorder="little")[: self.rows])
        assert span[0] == allowed[0] and span[1] == allowed[-1]
        return self._subset_batch(queries, allowed.astype(np.int64), k, thrs)


@pytest.fixture
def vb(monkeypatch):
    monkeypatch.setattr(_native, "Engine", MaskedFake)
    index = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    index.add_embeddings(None, make_corpus(N, D, 5200)[0])
    return index


def test_routing_between_the_gather_route_and_the_tile(vb):
    qs = make_queries(40, D, 5201)
    mask = np.zeros(N, dtype=bool)
    mask[300:650] = True
    handle = vb.row_mask(mask)
    eng = vb._sync_device()
    assert isinstance(handle, RowMask) and handle.span == (300, 649) and handle.dev_bits is not None and handle.count == 350
    want = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=10, min_score=0.0)
    assert [c[0] for c in eng.calls] == ["gather"]  # defaults: 350 x 128 bytes are far below mask_tile_min_bytes
    for setup, route in (((("mask_tile", 2),), "tile"), ((("mask_tile", 0),), "gather"), ((("mask_tile", 1), ("mask_tile_min_bytes", 0)), "tile"),
                         ((("mask_tile_min_bytes", 350 * 128 + 1),), "gather"), ((("mask_tile_min_bytes", 350 * 128),), "tile"),
                         ((("mask_tile_pct", 444),), "tile"), ((("mask_tile_pct", 445),), "gather")):  # 5 passes x 350 rows x 100 = 175000 against 1 tile x 394 rows x pct
        for name, val in setup:
            eng.set_option(name, val)
        eng.calls.clear()
        got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=10, min_score=0.0)
        assert [c[0] for c in eng.calls] == [route], (setup, eng.calls)
        assert got == want
    eng.set_option("mask_tile", 2)
    eng.set_option("mask_tile_pct", 100)
    eng.calls.clear()
    ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs[:3], mask, max_hits=64, min_score=[0.0, 0.5, 1.5], as_arrays=True)  # a raw mask, per-query thresholds
    assert eng.calls == [("tile", 3, 64, (300, 649))] and cnts.tolist()[0] == 64 and cnts[2] == 0 and mask[ords[0]].all()
    vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=65)  # beyond the tile's k: the gather route, whatever the option
    vb.fuzzy_lookup_embedding_masked(qs[0], handle, max_hits=5)
    assert [c[0] for c in eng.calls[1:]] == ["gather", "tile"]
    eng.calls.clear()
    assert vb.fuzzy_lookup_embeddings_masked(qs, np.zeros(N, dtype=bool)) == [[] for _ in qs] and eng.calls == []  # an empty mask calls nothing


def test_an_engine_without_the_new_calls_keeps_the_gather_route(monkeypatch):
    class Old(MaskedFake):
        search_masked_batch = None
        mask_to_rows_bits = None

        def __getattribute__(self, name):
            if name in ("search_masked_batch", "mask_to_rows_bits", "plan_masked"):
                raise AttributeError(name)
            return super().__getattribute__(name)

        def mask_to_rows(self, mask):
            flat = np.flatnonzero(np.asarray(mask)).astype(np.int32)
            return flat, len(flat)

    monkeypatch.setattr(_native, "Engine", Old)
    index = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    index.add_embeddings(None, make_corpus(N, D, 5200)[0])
    handle = index.row_mask(np.ones(N, dtype=bool))
    assert handle.dev_bits is None and handle.span is None
    eng = index._sync_device()
    eng.set_option("mask_tile", 2)
    index.fuzzy_lookup_embeddings_masked(make_queries(8, D, 1), handle, max_hits=10)
    assert [c[0] for c in eng.calls] == ["gather"]
