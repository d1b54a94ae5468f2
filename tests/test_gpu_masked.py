"""GPU suite: masked lookups (`VectorBase.row_mask`, `fuzzy_lookup_embedding(s)_masked`; tavb_mask_expand +
tavb_search_subset_batch_resident) -- every batch against the sequential subset lookups over np.flatnonzero(mask) on the same device
bit for bit (the library's invariant that a batch equals its sequential lookups), and against the oracle's subset lookup with
test_gpu_parity's rules (scores within 1e-5, near-ties decided by the float64 referee)."""

import numpy as np
import pytest
import torch

from oracle import vectorbase_oracle as vo
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

ROWS = 4097
NQS = [1, 2, 8, 9, 17]  # the group boundary at TAVB_MAX_STREAM_QUERIES and one group past it
MAX_HITS = [1, 10, 256, 300]  # 300: the large-k route
THR_CYCLE = [0.0, 0.5, 0.6, 0.45, 1.5, -0.2, 0.55, 0.52]
MASKS = ["random_0.02", "random_0.5", "all", "single", "none"]
_cache: dict = {}


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def setup(d: int, dtype: str, rows: int = ROWS):
    """(index, the rows as the kernels see them, queries) -- built once per shape and left unchanged"""
    key = (d, dtype, rows)
    if key not in _cache:
        v, _ = make_corpus(rows, d, 5100 + d)
        qs = make_queries(max(NQS), d, 5200 + d)
        qs[3] = v[rows // 2]  # a query equal to a row: something passes 0.6 at every width
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        vb.add_embeddings(None, v)
        _cache[key] = (vb, _f16(v) if dtype == "fp16" else v, qs)
    return _cache[key]


def make_mask(kind: str, rows: int) -> np.ndarray:
    m = np.zeros(rows, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "single":
        m[rows // 2] = True
    elif kind.startswith("random_"):
        m = np.random.default_rng(rows + 7).random(rows) < float(kind.split("_")[1])
        m[rows // 2] = True
    return m


def pairs(res):
    assert all(isinstance(r, ScoredInt) for r in res)
    return [r.item for r in res], [r.score for r in res]


def assert_same(a, b, what):
    """two hit lists equal bit for bit: ordinals, float32 score bits, length"""
    (ia, sa), (ib, sb) = pairs(a), pairs(b)
    assert ia == ib, what
    assert np.asarray(sa, dtype=np.float32).view(np.uint32).tolist() == np.asarray(sb, dtype=np.float32).view(np.uint32).tolist(), what


def assert_oracle(res, flat, referee, sub_scores, k, ms):
    """the oracle's subset lookup over `flat` (its scores: sub_scores) by test_gpu_parity's rules: ordinals identical, scores within 1e-5,
    near-ties decided by the float64 referee"""
    items, scores = pairs(res)
    if len(flat) == 0:
        assert items == []
        return
    vo.check_topk_parity(sub_scores, items, scores, k, ms, candidate_ordinals=flat, referee=referee)


def run_case(vb, vv, qs, mask, nqs=NQS, max_hits=MAX_HITS):
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.count == len(flat) and handle.rows == len(vb)
    sub = vv[flat]  # the reference, computed once
    sub_scores = [vo.cosine_to_score(np.dot(sub, q)) for q in qs]
    referees = [vo.f64_referee(sub, q) for q in qs]
    for k in max_hits:
        for ms in (0.0, 0.6, "per_query"):
            thr = (lambda i: THR_CYCLE[i % len(THR_CYCLE)]) if ms == "per_query" else (lambda i: ms)
            seq = [vb.fuzzy_lookup_embedding_in_subset(q, flat, max_hits=k, min_score=thr(i)) for i, q in enumerate(qs)]
            for nq in nqs:
                arg = [thr(i) for i in range(nq)] if ms == "per_query" else ms
                got = vb.fuzzy_lookup_embeddings_masked(qs[:nq], handle if nq % 2 else mask, max_hits=k, min_score=arg)
                assert len(got) == nq
                for i in range(nq):
                    assert_same(got[i], seq[i], (k, ms, nq, i))
                    assert_oracle(got[i], flat, referees[i], sub_scores[i], k, thr(i))
                if len(flat) == 0:
                    assert got == [[] for _ in range(nq)]
            if ms != "per_query":
                assert_same(vb.fuzzy_lookup_embedding_masked(qs[3], handle, max_hits=k, min_score=ms), seq[3], (k, ms, "single"))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [1536, 384, 50])  # the fixed, vector and scalar tiers of the streaming scan
def test_masked_batches_equal_sequential_subset_lookups_and_the_oracle(d, dtype, kind):
    vb, vv, qs = setup(d, dtype)
    run_case(vb, vv, qs, make_mask(kind, ROWS))


def test_expansion_and_scan_spanning_several_workgroups():
    rows = 70_001
    assert rows > 4 * _native.MASK_ROWS_PER_WORKGROUP
    vb, vv, qs = setup(384, "fp16", rows)
    run_case(vb, vv, qs, make_mask("random_0.5", rows), nqs=[9], max_hits=[10, 300])


def test_ties_come_back_in_ascending_ordinal_order():
    d = 384
    base, _ = make_corpus(50, d, 5300)
    v = base[np.arange(ROWS) % 50]  # every row 81 or 82 times
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb.add_embeddings(None, v)
    mask = make_mask("random_0.5", ROWS)
    flat = np.flatnonzero(mask)
    qs = np.stack([v[7], v[11], v[49]])
    for k in (1, 10, 256, 300):
        got = vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=k, min_score=0.0)
        for i, src in enumerate((7, 11, 49)):
            items, scores = pairs(got[i])
            assert len(items) == k
            twins = flat[flat % 50 == src]  # the allowed copies of the query's row, ascending: all score 1.0 (to rounding) and tie exactly
            lead = min(k, len(twins))
            assert items[:lead] == twins[:lead].tolist()
            assert len(set(scores[:lead])) == 1
            for j in range(1, k):  # everywhere: score descending, equal scores by ascending ordinal
                assert scores[j - 1] > scores[j] or (scores[j - 1] == scores[j] and items[j - 1] < items[j])
            assert_same(got[i], vb.fuzzy_lookup_embedding_in_subset(qs[i], flat, max_hits=k, min_score=0.0), (k, i))


def test_handle_arrays_device_masks_and_the_fallback_route():
    vb, vv, qs = setup(384, "fp32")
    mask = make_mask("random_0.5", ROWS)
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    want = vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=10, min_score=0.0)
    for _ in range(3):  # a RowMask reused across calls
        assert vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=10, min_score=0.0) == want
    np.testing.assert_array_equal(handle.flat(), flat)
    # a mask made on the device never visits the host
    dev_mask = torch.from_numpy(mask).to(f"cuda:{vb.engine.device}")
    dev_handle = vb.row_mask(dev_mask)
    assert dev_handle.count == len(flat) and torch.equal(dev_handle.dev_rows, handle.dev_rows)
    assert vb.fuzzy_lookup_embeddings_masked(qs, dev_mask, max_hits=10, min_score=0.0) == want
    assert vb.fuzzy_lookup_embeddings_masked(qs, torch.from_numpy(mask), max_hits=10, min_score=0.0) == want  # a host tensor: as an array
    # as_arrays matches the lists
    ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=10, min_score=0.0, as_arrays=True)
    assert ords.shape == scs.shape == (len(qs), 10) and cnts.tolist() == [len(h) for h in want]
    for i, hits in enumerate(want):
        assert ords[i, : cnts[i]].tolist() == [h.item for h in hits]
        assert scs[i, : cnts[i]].tolist() == [np.float32(h.score) for h in hits]
    # max_hits == 0 (every survivor): the fallback, same answers as the subset lookup and the oracle
    for ms in (0.0, 0.52):
        got = vb.fuzzy_lookup_embeddings_masked(qs[:3], handle, max_hits=0, min_score=ms)
        for i in range(3):
            assert_same(got[i], vb.fuzzy_lookup_embedding_in_subset(qs[i], flat, max_hits=0, min_score=ms), (0, ms, i))
            assert_oracle(got[i], flat, vo.f64_referee(vv[flat], qs[i]), vo.cosine_to_score(np.dot(vv[flat], qs[i])), 0, ms)
    # positions instead of ordinals (remap off) index the row list
    o0, s0, c0 = vb.engine.search_subset_batch_resident(qs[:2], handle.dev_rows, 10, 0.0, remap=False)
    o1, s1, c1 = vb.engine.search_subset_batch_resident(qs[:2], handle.dev_rows, 10, 0.0, remap=True)
    np.testing.assert_array_equal(flat[o0], o1)
    np.testing.assert_array_equal(s0, s1)
    # ... also where the keys are merged in device memory and copied out once (more than 4096 of them)
    o0, s0, c0 = vb.engine.search_subset_batch_resident(qs, handle.dev_rows, 256, 0.0, remap=False)
    o1, s1, c1 = vb.engine.search_subset_batch_resident(qs, handle.dev_rows, 256, 0.0, remap=True)
    assert c0.tolist() == c1.tolist() == [256] * len(qs)
    np.testing.assert_array_equal(flat[o0], o1)
    np.testing.assert_array_equal(s0, s1)
    # "large_k" off: max_hits beyond 256 leaves the top-k kernels, as for every other lookup, with the same answers
    want300 = vb.fuzzy_lookup_embeddings_masked(qs[:3], handle, max_hits=300, min_score=0.0)
    vb.engine.set_option("large_k", 0)
    try:
        got300 = vb.fuzzy_lookup_embeddings_masked(qs[:3], handle, max_hits=300, min_score=0.0)
    finally:
        vb.engine.set_option("large_k", 1)
    for i in range(3):
        assert_same(got300[i], want300[i], ("large_k off", i))
    # stale after the index grew
    grown = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    grown.add_embeddings(None, vv[:100])
    h = grown.row_mask(mask[:100])
    grown.add_embedding(None, vv[100])
    with pytest.raises(ValueError, match="mask covers 100 rows, the index has 101"):
        grown.fuzzy_lookup_embedding_masked(qs[0], h)
