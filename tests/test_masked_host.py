"""CPU suite: the masked lookups of the drop-in class on their fallback route (the numpy engine double of tests/fake_engine.py) against
the oracle's subset lookup over np.flatnonzero(mask), their argument errors, and the host packing of a mask into the bit form
tavb_mask_expand reads (row r = bit r & 31 of word r >> 5)."""

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native

N, D = 200, 32


@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 4100)
    return v, make_queries(5, D, 4101)


@pytest.fixture
def vb(monkeypatch, corpus):
    monkeypatch.setattr(_native, "Engine", FakeEngine)
    index = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    index.add_embeddings(None, corpus[0])
    return index


def masks():
    rng = np.random.default_rng(4102)
    one = np.zeros(N, dtype=bool)
    one[137] = True
    return {"none": np.zeros(N, dtype=bool), "all": np.ones(N, dtype=bool), "one": one, "random": rng.random(N) < 0.3}


def same(res, ref):
    assert all(isinstance(r, ScoredInt) for r in res)
    assert [r.item for r in res] == [i for i, _ in ref]
    np.testing.assert_allclose([r.score for r in res], [s for _, s in ref], atol=1e-6, rtol=0)


@pytest.mark.parametrize("name", ["none", "all", "one", "random"])
@pytest.mark.parametrize("max_hits", [None, 1, 10, 0])
def test_fallback_equals_the_oracle_subset_lookup(vb, corpus, name, max_hits):
    v, qs = corpus
    mask = masks()[name]
    flat = np.flatnonzero(mask).tolist()
    per_query = [0.0, 0.5, 0.45, 0.55, 1.5]
    for min_score in (None, 0.5, per_query):
        got = vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=max_hits, min_score=min_score)
        assert len(got) == len(qs)
        for i, q in enumerate(qs):
            ms = min_score[i] if isinstance(min_score, list) else min_score
            ref = vo.lookup_in_subset(v, q, flat, max_hits, ms)
            same(got[i], ref)
            if not isinstance(min_score, list):
                same(vb.fuzzy_lookup_embedding_masked(q, mask, max_hits=max_hits, min_score=ms), ref)
        if name == "none":
            assert got == [[] for _ in qs]


def test_a_row_mask_is_reused_and_a_sequence_is_a_mask(vb, corpus):
    v, qs = corpus
    mask = masks()["random"]
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.rows == N and handle.count == len(handle) == int(mask.sum())
    np.testing.assert_array_equal(handle.flat(), np.flatnonzero(mask))
    first = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=7, min_score=0.4)
    assert first == vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=7, min_score=0.4) == vb.fuzzy_lookup_embeddings_masked(qs, mask.tolist(), 7, 0.4)
    ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=7, min_score=0.4, as_arrays=True)
    assert ords.shape == scs.shape == (len(qs), 7) and ords.dtype == np.int64 and scs.dtype == np.float32 and cnts.dtype == np.int32
    for i, hits in enumerate(first):
        assert cnts[i] == len(hits) and ords[i, : cnts[i]].tolist() == [h.item for h in hits]
        assert scs[i, : cnts[i]].tolist() == [np.float32(h.score) for h in hits]


def test_argument_errors(vb, corpus):
    v, qs = corpus
    mask = masks()["random"]
    with pytest.raises(ValueError, match=f"mask covers {N - 1} rows, the index has {N}"):
        vb.row_mask(mask[:-1])
    with pytest.raises(ValueError, match=f"mask covers {N + 1} rows, the index has {N}"):
        vb.fuzzy_lookup_embedding_masked(qs[0], np.ones(N + 1, dtype=bool))
    for bad in (mask.astype(np.uint8), mask.astype(np.int64), np.flatnonzero(mask), mask.astype(np.float32)):
        with pytest.raises(TypeError):
            vb.row_mask(bad)
        with pytest.raises(TypeError):
            vb.fuzzy_lookup_embeddings_masked(qs, bad)
    with pytest.raises(ValueError, match="Expected 2D embeddings array, got 1D"):
        vb.fuzzy_lookup_embeddings_masked(qs[0], mask)
    with pytest.raises(ValueError):
        vb.fuzzy_lookup_embedding_masked(qs, mask)
    with pytest.raises(ValueError, match="Number of thresholds"):
        vb.fuzzy_lookup_embeddings_masked(qs, mask, min_score=[0.1, 0.2])
    with pytest.raises(ValueError, match="max_hits must be >= 0"):
        vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=-1)
    with pytest.raises(ValueError, match="as_arrays"):
        vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=0, as_arrays=True)


def test_a_stale_row_mask_is_refused(vb, corpus, monkeypatch):
    v, qs = corpus
    handle = vb.row_mask(masks()["random"])
    assert len(vb.fuzzy_lookup_embedding_masked(qs[0], handle, max_hits=3)) == 3
    vb.add_embedding(None, v[0])  # grew
    with pytest.raises(ValueError, match=f"mask covers {N} rows, the index has {N + 1}"):
        vb.fuzzy_lookup_embedding_masked(qs[0], handle)
    with pytest.raises(ValueError, match=f"mask covers {N} rows, the index has {N + 1}"):
        vb.fuzzy_lookup_embeddings_masked(qs, handle)
    vb.clear()  # shrank
    with pytest.raises(ValueError, match="the index has 0"):
        vb.fuzzy_lookup_embedding_masked(qs[0], handle)
    other = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    other.add_embeddings(None, v)
    with pytest.raises(ValueError, match="another index"):
        other.fuzzy_lookup_embedding_masked(qs[0], handle)
    empty = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    assert empty.fuzzy_lookup_embeddings_masked(np.zeros((2, D), np.float32), np.zeros(0, dtype=bool)) == [[], []]


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 65])
def test_packing_puts_row_r_at_bit_r_and_31_of_word_r_shift_5(rows):
    rng = np.random.default_rng(rows)
    for mask in (np.ones(rows, dtype=bool), np.zeros(rows, dtype=bool), rng.random(rows) < 0.5, np.arange(rows) == rows - 1):
        words = _native.pack_mask_bits(mask)
        assert words.dtype == np.uint32 and words.shape == ((rows + 31) // 32,)
        for r in range(rows):
            assert bool((int(words[r >> 5]) >> (r & 31)) & 1) == bool(mask[r]), (rows, r)
        for r in range(rows, 32 * len(words)):  # the tail of the last word is zero
            assert not (int(words[r >> 5]) >> (r & 31)) & 1
    with pytest.raises(TypeError):
        _native.pack_mask_bits(np.ones(rows, dtype=np.uint8))


def test_the_workgroup_chunk_matches_the_header_and_the_null_context_is_refused():
    import ctypes
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "tavb.h")).read()
    assert _native.MASK_ROWS_PER_WORKGROUP == int(re.search(r"#define TAVB_MASK_ROWS_PER_WORKGROUP (\d+)", text).group(1))
    assert _native.MASK_ROWS_PER_WORKGROUP % (32 * 256) == 0  # whole rounds of a 256-thread workgroup, one word per thread
    lib = _native.load_library(preload_torch=False)
    cnt = ctypes.c_int64(5)
    assert lib.tavb_mask_expand(None, None, 10, None, 0, ctypes.byref(cnt)) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_mask_pack(None, None, 10, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_subset_batch_resident(None, None, 1, None, 1, 10, None, 1, None, None, None) == -1
    assert b"null context" in lib.tavb_last_error()


def test_a_sharded_index_takes_the_fallback(corpus):
    """ShardedVectorBase has no masked route of its own: its masked lookups are the (collective) subset lookup per query over
    np.flatnonzero(mask), with the same argument errors.  The subset lookup itself is replaced by a recorder here."""
    from typeagent_py_amd.sharded import ShardedVectorBase

    calls = []

    class Recorder(ShardedVectorBase):
        def __init__(self, total):
            self.total_rows = total

        def fuzzy_lookup_embedding_in_subset(self, embedding, ordinals_of_subset, max_hits=None, min_score=None):
            calls.append((np.asarray(embedding).tolist(), np.asarray(ordinals_of_subset).tolist(), max_hits, min_score))
            return [ScoredInt(int(ordinals_of_subset[0]), 1.0)] if len(ordinals_of_subset) else []

    v, qs = corpus
    svb = Recorder(N)
    mask = masks()["random"]
    flat = np.flatnonzero(mask).tolist()
    handle = svb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.count == len(flat)
    got = svb.fuzzy_lookup_embeddings_masked(qs[:3], handle, max_hits=4, min_score=[0.1, 0.2, 0.3])
    assert got == [[ScoredInt(flat[0], 1.0)]] * 3
    assert calls == [(qs[i].tolist(), flat, 4, ms) for i, ms in enumerate([0.1, 0.2, 0.3])]
    calls.clear()
    assert svb.fuzzy_lookup_embedding_masked(qs[0], mask, max_hits=0, min_score=0.5) == [ScoredInt(flat[0], 1.0)]
    assert calls == [(qs[0].tolist(), flat, 0, 0.5)]
    with pytest.raises(ValueError, match=f"mask covers {N - 1} rows, the index has {N}"):
        svb.row_mask(mask[:-1])
    with pytest.raises(TypeError):
        svb.fuzzy_lookup_embedding_masked(qs[0], mask.astype(np.uint8))
    with pytest.raises(ValueError, match="Expected 2D"):
        svb.fuzzy_lookup_embeddings_masked(qs[0], mask)
    svb.total_rows = N + 1
    with pytest.raises(ValueError, match=f"mask covers {N} rows, the index has {N + 1}"):
        svb.fuzzy_lookup_embedding_masked(qs[0], handle)
    with pytest.raises(ValueError, match="another index"):
        Recorder(N).fuzzy_lookup_embedding_masked(qs[0], handle)
