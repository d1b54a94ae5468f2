"""CPU suite: the masked route of device groups (`DeviceGroup.mask_to_rows` / `search_masked` under `VectorBase(devices=[...])`) and of
row-sharded indexes (`ShardedVectorBase` over a backend that offers `mask_to_device` / `local_search_masked`) with numpy doubles defined
here: which route a lookup takes, what every shard is handed, how many exchanges a batch costs, and that the answers are the fallback's and
the oracle subset lookup's.  Plus the new symbol in the header and the binding, and its null-context error."""

import os
import re

import numpy as np
import pytest
import torch

from oracle import vectorbase_oracle as vo
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from tests.test_sharded_large_k_host import NumpyShardBackend
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native
from typeagent_py_amd.multidevice import DeviceGroup
from typeagent_py_amd.sharded import PeerFailedError, ShardedVectorBase

N, D = 200, 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 4300)
    return v, make_queries(5, D, 4301)


def masks():
    rng = np.random.default_rng(4302)
    one = np.zeros(N, dtype=bool)
    one[171] = True
    no_middle = rng.random(N) < 0.4
    no_middle[67:134] = False
    return {"none": np.zeros(N, dtype=bool), "all": np.ones(N, dtype=bool), "one": one, "random": rng.random(N) < 0.3, "no_middle": no_middle}


def same(res, ref):
    assert all(isinstance(r, ScoredInt) for r in res)
    assert [r.item for r in res] == [i for i, _ in ref]
    np.testing.assert_allclose([r.score for r in res], [s for _, s in ref], atol=1e-6, rtol=0)


# ---- doubles -------------------------------------------------------------------------------------------------------------------------

class MaskedFakeEngine(FakeEngine):
    """FakeEngine + the two calls a masked-capable engine offers (CPU tensors stand in for device memory).  TEST ONLY."""

    def __init__(self, device=None, use_torch_stream=False):
        super().__init__(device, use_torch_stream)
        self.options["large_k"] = 1
        self.mask_slices: list = []
        self.batch_calls: list = []  # (nq, rows, k) per search_subset_batch_device call

    def synchronize(self):
        pass

    def search_topk_device(self, *a, **kw):  # (what `large_k_capable` looks for; these tests never reach it)
        raise AssertionError("not expected here")

    def rows_to_device(self, rows):
        return torch.from_numpy(np.array(rows, dtype=np.int32))

    def mask_to_rows(self, mask):
        m = np.asarray(mask)
        assert m.dtype == np.bool_ and m.shape == (self.rows,)
        self.mask_slices.append(m.copy())
        rows = np.flatnonzero(m).astype(np.int32)
        return torch.from_numpy(rows), len(rows)

    def search_subset_batch_device(self, dev_queries, dev_rows, k, thrs, out_keys=None, remap=True):
        q = dev_queries.numpy()
        rows = dev_rows.numpy().astype(np.int64)
        assert remap and len(rows) and (np.diff(rows) > 0).all() and rows[-1] < self.rows
        t = np.broadcast_to(np.asarray(thrs, dtype=np.float32), (len(q),))
        self.batch_calls.append((len(q), len(rows), k))
        keys = np.zeros((len(q), k), dtype=np.uint64)
        for i in range(len(q)):
            pos, sc = self.search_subset(q[i], rows, k, t[i])
            keys[i, : len(pos)] = (sc.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - (rows[pos] + self.ordinal_base).astype(np.uint64))
        self._write(out_keys, keys)
        return out_keys


def group_index(monkeypatch, engine_cls, rows):
    monkeypatch.setattr(_native, "Engine", engine_cls)
    # (pinned and device buffers need a GPU: plain CPU tensors stand in for both)
    monkeypatch.setattr(DeviceGroup, "_topk_lists", lambda self, shards, nq, k: torch.zeros((shards, nq, k), dtype=torch.int64))
    monkeypatch.setattr(DeviceGroup, "_device_queries", lambda self, shards, a: [torch.from_numpy(a) for _ in shards])
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 1, 2])
    vb.add_embeddings(None, rows)
    return vb


# ---- device groups -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["none", "all", "one", "random", "no_middle"])
def test_a_group_of_masked_capable_engines_takes_the_route(monkeypatch, corpus, name):
    v, qs = corpus
    vb = group_index(monkeypatch, MaskedFakeEngine, v)
    geng = vb._sync_device()
    assert geng.masked_capable() and list(geng.bounds) == [0, 67, 134, 200]
    mask = masks()[name]
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.count == len(flat) and handle.bounds == (0, 67, 134, 200)
    np.testing.assert_array_equal(handle.flat(), flat)
    for g, e in enumerate(geng.engines):  # every shard saw ITS slice of the mask, once
        assert len(e.mask_slices) == 1
        np.testing.assert_array_equal(e.mask_slices[0], mask[geng.bounds[g] : geng.bounds[g + 1]])
        assert (handle.shards[g] is None) == (not mask[geng.bounds[g] : geng.bounds[g + 1]].any())
    per_query = [0.0, 0.5, 0.45, 0.55, 1.5]
    lookups = 0
    for max_hits in (None, 1, 10, 300):
        for min_score in (None, 0.5, per_query):
            got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=max_hits, min_score=min_score)
            lookups += 1 if len(flat) else 0
            for i, q in enumerate(qs):
                ms = min_score[i] if isinstance(min_score, list) else min_score
                same(got[i], vo.lookup_in_subset(v, q, flat.tolist(), max_hits, ms))
    for g, e in enumerate(geng.engines):  # ONE batched call per lookup on every shard that has allowed rows, none elsewhere
        has = handle.shards[g] is not None
        assert len(e.batch_calls) == (lookups if has else 0)
        assert all(nq == len(qs) and n == len(handle.shards[g]) for nq, n, k in e.batch_calls)
    if len(flat):
        ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=7, min_score=0.4, as_arrays=True)
        lists = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=7, min_score=0.4)
        assert ords.shape == scs.shape == (len(qs), 7) and cnts.tolist() == [len(h) for h in lists]
        for i, hits in enumerate(lists):
            assert ords[i, : cnts[i]].tolist() == [h.item for h in hits] and scs[i, : cnts[i]].tolist() == [np.float32(h.score) for h in hits]


def test_the_route_equals_the_fallback_and_what_it_does_not_take_keeps_the_fallback(monkeypatch, corpus):
    v, qs = corpus
    mask = masks()["random"]
    flat = np.flatnonzero(mask)
    plain = group_index(monkeypatch, FakeEngine, v)  # a group of plain doubles: no route, np.flatnonzero in the handle
    assert not plain._sync_device().masked_capable()
    plain_handle = plain.row_mask(mask)
    assert plain_handle.shards is None
    np.testing.assert_array_equal(plain_handle.flat(), flat)
    vb = group_index(monkeypatch, MaskedFakeEngine, v)
    geng = vb._sync_device()
    handle = vb.row_mask(mask)
    thr = [0.0, 0.5, 0.45, 0.55, 1.5]
    for max_hits in (1, 10, 256):
        assert vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits, thr) == plain.fuzzy_lookup_embeddings_masked(qs, plain_handle, max_hits, thr)
    routed = sum(len(e.batch_calls) for e in geng.engines)
    assert routed == 3 * 3
    for max_hits in (0, 20000):  # every survivor, and more hits than the exact top-k serves: the per-query fallback
        got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits, thr)
        assert got == plain.fuzzy_lookup_embeddings_masked(qs, plain_handle, max_hits, thr)
        for i, q in enumerate(qs):
            same(got[i], vo.lookup_in_subset(v, q, flat.tolist(), max_hits, thr[i]))
    on = vb.fuzzy_lookup_embeddings_masked(qs, handle, 300, thr)
    assert sum(len(e.batch_calls) for e in geng.engines) == routed + 3
    geng.set_option("large_k", 0)  # the switch of every other lookup beyond 256
    assert vb.fuzzy_lookup_embeddings_masked(qs, handle, 300, thr) == on
    assert sum(len(e.batch_calls) for e in geng.engines) == routed + 3
    # the checks on a handle stay: another index, another length
    with pytest.raises(ValueError, match="another index"):
        plain.fuzzy_lookup_embeddings_masked(qs, handle)
    vb.add_embedding(None, v[0])
    with pytest.raises(ValueError, match=f"mask covers {N} rows, the index has {N + 1}"):
        vb.fuzzy_lookup_embeddings_masked(qs, handle)


def test_a_handle_cut_under_other_bounds_is_cut_again(monkeypatch, corpus):
    v, qs = corpus
    vb = group_index(monkeypatch, MaskedFakeEngine, v[:150])
    geng = vb._sync_device()
    vb.add_embeddings(None, v[150:])  # grown: the last shard takes the appends
    mask = masks()["random"]
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    assert handle.bounds == tuple(geng.bounds) == (0, 50, 100, 200)
    before = vb.fuzzy_lookup_embeddings_masked(qs, handle, 10, 0.4)
    vb.mark_dirty()  # the next lookup uploads from row 0: balanced shards, the same length
    after = vb.fuzzy_lookup_embeddings_masked(qs, handle, 10, 0.4)
    assert tuple(geng.bounds) == (0, 67, 134, 200) and handle.bounds == (0, 67, 134, 200)
    for a, b in zip(after, before):  # (the doubles' BLAS sums a row's products in another order once the shard around it changes)
        same(a, [(h.item, h.score) for h in b])
    for i, q in enumerate(qs):
        same(after[i], vo.lookup_in_subset(v, q, flat.tolist(), 10, 0.4))
    np.testing.assert_array_equal(handle.flat(), flat)
    for g, e in enumerate(geng.engines):
        np.testing.assert_array_equal(handle.shards[g].numpy(), np.flatnonzero(mask[geng.bounds[g] : geng.bounds[g + 1]]))
        assert len(e.mask_slices) == 1  # cut from flat(), not expanded again
    assert vb.fuzzy_lookup_embeddings_masked(qs, handle, 10, 0.4) == after


# ---- row-sharded indexes (world 1) ---------------------------------------------------------------------------------------------------

class MaskedNumpyBackend(NumpyShardBackend):
    """NumpyShardBackend + the two calls of the masked route.  TEST ONLY."""

    def __init__(self, shard, row_offset, fail=False):
        super().__init__(shard, row_offset, fail)
        self.expansions = 0
        self.masked_calls: list = []

    def mask_to_device(self, local_mask):
        m = np.asarray(local_mask)
        assert m.dtype == np.bool_ and m.shape == (len(self.shard),)
        self.expansions += 1
        rows = np.flatnonzero(m)
        return rows if len(rows) else None

    def local_search_masked(self, queries, handle, k, thrs):
        self.masked_calls.append((len(queries), 0 if handle is None else len(handle), k))
        if handle is None:
            return torch.zeros((len(queries), k), dtype=torch.int64)
        keys = [self._local(self.shard[handle], handle + self.row_offset, q, k, thrs[i]) for i, q in enumerate(queries)]
        return torch.from_numpy(np.stack(keys).view(np.int64))


def sharded_index(v, row_offset=0, local_rows=None, total=None, backend_cls=MaskedNumpyBackend):
    local_rows = len(v) - row_offset if local_rows is None else local_rows
    backend = backend_cls(v[row_offset : row_offset + local_rows], row_offset)
    svb = ShardedVectorBase(backend, row_offset, local_rows, len(v) if total is None else total)
    exchanges = []
    inner = svb.searcher.exchange
    svb.searcher.exchange = lambda keys: (exchanges.append(tuple(keys.shape)), inner(keys))[1]
    return svb, backend, exchanges


def test_a_sharded_index_takes_the_masked_route_with_one_exchange_per_batch(corpus):
    v, qs = corpus
    svb, backend, exchanges = sharded_index(v)
    thr = [0.0, 0.5, 0.45, 0.55, 1.5]
    for name in ("all", "one", "random"):
        mask = masks()[name]
        flat = np.flatnonzero(mask)
        handle = svb.row_mask(mask)
        assert isinstance(handle, RowMask) and handle.count == len(flat) and handle.layout == (N, 0, N)
        np.testing.assert_array_equal(handle.bits, _native.pack_mask_bits(mask))
        np.testing.assert_array_equal(handle.flat(), flat)
        for max_hits in (None, 3, 300):
            for min_score in (None, 0.5, thr):
                exchanges.clear()
                backend.masked_calls.clear()
                got = svb.fuzzy_lookup_embeddings_masked(qs, handle if max_hits else mask, max_hits, min_score)
                k = 10 if max_hits is None else max_hits
                assert exchanges == [(len(qs), k)] and backend.masked_calls == [(len(qs), len(flat), k)]  # ONE local call, ONE exchange
                want = [svb.fuzzy_lookup_embedding_in_subset(e, flat, max_hits, min_score[i] if isinstance(min_score, list) else min_score) for i, e in enumerate(qs)]
                assert got == want
                for i, q in enumerate(qs):
                    same(got[i], vo.lookup_in_subset(v, q, flat.tolist(), max_hits, min_score[i] if isinstance(min_score, list) else min_score))
        assert svb.fuzzy_lookup_embedding_masked(qs[0], handle, 4, 0.3) == svb.fuzzy_lookup_embedding_in_subset(qs[0], flat, 4, 0.3)
    # a globally empty mask, an empty batch: empty lists, nothing exchanged
    exchanges.clear()
    assert svb.fuzzy_lookup_embeddings_masked(qs, masks()["none"], 5) == [[] for _ in qs]
    assert svb.fuzzy_lookup_embeddings_masked(qs[:0], masks()["random"], 5) == []
    assert exchanges == []
    for bad in (0, 20000):
        with pytest.raises(ValueError, match="1..16384"):
            svb.fuzzy_lookup_embeddings_masked(qs, masks()["random"], max_hits=bad)
    with pytest.raises(ValueError, match=f"mask covers {N - 1} rows, the index has {N}"):
        svb.row_mask(masks()["random"][:-1])
    with pytest.raises(TypeError):
        svb.row_mask(masks()["random"].astype(np.uint8))
    with pytest.raises(ValueError, match="Number of thresholds"):
        svb.fuzzy_lookup_embeddings_masked(qs, masks()["random"], 5, [0.1, 0.2])
    assert exchanges == []


def test_an_empty_local_part_still_exchanges_and_a_raising_one_follows_the_protocol(corpus):
    v, qs = corpus
    svb, backend, exchanges = sharded_index(v, row_offset=0, local_rows=100, total=N)  # as rank 0 of two would hold it
    mask = np.zeros(N, dtype=bool)
    mask[150:160] = True  # allowed rows only in the other rank's part
    handle = svb.row_mask(mask)
    assert handle.count == 10 and handle.dev_rows is None
    assert svb.fuzzy_lookup_embeddings_masked(qs, handle, 5) == [[] for _ in qs]  # (this rank's part of the answer: nothing)
    assert exchanges == [(len(qs), 5)] and backend.masked_calls == [(len(qs), 0, 5)]
    # a local part that raises still joins the exchange -- with the failure lists -- and raises its own error afterwards
    svb, backend, exchanges = sharded_index(v)
    backend.native_comm = True  # (a communicator: the protocol applies even to a world of one)
    svb.searcher.gather_fn = lambda local: local[None]
    handle = svb.row_mask(masks()["random"])
    backend.fail = True
    with pytest.raises(RuntimeError, match="injected failure"):
        svb.fuzzy_lookup_embeddings_masked(qs, handle, 5)
    assert exchanges == [(len(qs), 5)]
    backend.fail = False
    svb.searcher.gather_fn = lambda local: torch.stack([local, torch.full_like(local, -1)])  # a peer that failed
    with pytest.raises(PeerFailedError):
        svb.fuzzy_lookup_embeddings_masked(qs, handle, 5)
    svb.searcher.gather_fn = lambda local: local[None]
    assert svb.fuzzy_lookup_embeddings_masked(qs, handle, 5) == [svb.fuzzy_lookup_embedding_in_subset(q, handle.flat(), 5) for q in qs]


@pytest.mark.parametrize("layout", [(0, 120), (13, 150), (64, 136), (77, 0)])
def test_a_handle_cut_under_another_layout_is_cut_again_from_its_bits(corpus, layout):
    v, qs = corpus
    svb, backend, exchanges = sharded_index(v)
    mask = masks()["random"]
    handle = svb.row_mask(mask)
    assert backend.expansions == 1
    # the rows are re-dealt (what rebalance() does to this rank): another offset and count, the same total
    lo, n = layout
    backend.shard, backend.row_offset = v[lo : lo + n], lo
    svb.row_offset, svb.local_rows = lo, n
    got = svb.fuzzy_lookup_embeddings_masked(qs, handle, 7, 0.3)
    assert backend.expansions == 2 and handle.layout == (N, lo, n)
    mine = np.flatnonzero(mask[lo : lo + n])
    assert (handle.dev_rows is None and len(mine) == 0) or np.array_equal(handle.dev_rows, mine)
    assert got == [svb.fuzzy_lookup_embedding_in_subset(q, np.flatnonzero(mask), 7, 0.3) for q in qs]
    assert svb.fuzzy_lookup_embeddings_masked(qs, handle, 7, 0.3) == got and backend.expansions == 2  # cut once
    np.testing.assert_array_equal(handle.flat(), np.flatnonzero(mask))


def test_a_backend_without_the_methods_keeps_the_per_query_fallback(corpus):
    v, qs = corpus
    svb, backend, exchanges = sharded_index(v, backend_cls=NumpyShardBackend)
    mask = masks()["random"]
    handle = svb.row_mask(mask)
    assert handle.bits is None and handle.layout is None
    got = svb.fuzzy_lookup_embeddings_masked(qs, handle, 5, 0.2)
    assert len(exchanges) == len(qs)  # one exchange per query
    assert got == [svb.fuzzy_lookup_embedding_in_subset(q, np.flatnonzero(mask), 5, 0.2) for q in qs]


# ---- symbols and arguments -----------------------------------------------------------------------------------------------------------

def test_the_new_symbol_is_declared_bound_and_refuses_a_null_context():
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(tavb_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_native.ABI_SYMBOLS)
    assert "tavb_search_subset_batch_device" in declared
    lib = _native.load_library(preload_torch=False)
    assert lib.tavb_version() == 7  # additive: the ABI version stays
    assert lib.tavb_search_subset_batch_device(None, None, 1, None, 1, 10, None, 1, None) == -1
    assert b"null context" in lib.tavb_last_error()
