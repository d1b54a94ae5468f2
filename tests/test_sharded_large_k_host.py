"""CPU suite: max_hits 257 .. 16384 on row-sharded indexes.

  * `tavb_merge_topk_host` (`_native.merge_topk_keys`), the host merge of long sorted lists, against a plain descending sort of the union;
  * `ShardedVectorBase` over gloo with world 2 and 3 and a numpy backend of this file's own: the plain, batched and subset lookups at
    max_hits 300 and 1000 equal the oracle over the whole corpus, a failing rank raises on itself and `PeerFailedError` everywhere else;
  * max_hits 0 and 20000 still raise on the SPMD form.

No GPU: the host merge is a pure host helper of libtavb.so, and the backend's local search is the oracle."""

import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILED = np.uint64(0xFFFFFFFFFFFFFFFF)


def make_lists(rng, n_lists: int, nq: int, k: int, fill: str = "full") -> np.ndarray:
    """uint64 [n_lists, nq, k]: sorted (descending), zero-padded lists of UNIQUE keys (score bits << 32 | 0xFFFFFFFF - ordinal).
    fill: "full" = k keys per list, "ragged" = 0 .. k keys per list (some lists empty), "empty" = no key at all."""
    lists = np.zeros((n_lists, nq, k), dtype=np.uint64)
    if fill == "empty":
        return lists
    for q in range(nq):
        lens = np.full(n_lists, k) if fill == "full" else rng.integers(0, k + 1, size=n_lists)
        if fill == "ragged":
            lens[rng.integers(0, n_lists)] = 0
        total = int(lens.sum())
        # few distinct scores: most of the order is decided by the ordinal half of the keys
        scores = rng.choice(np.linspace(0.0, 1.0, 97, dtype=np.float32), size=total)
        ords = rng.permutation(max(total, 1) * 3)[:total].astype(np.uint64)
        keys = (scores.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ords)
        at = 0
        for l in range(n_lists):
            part = np.sort(keys[at : at + lens[l]])[::-1]
            lists[l, q, : lens[l]] = part
            at += lens[l]
    return lists


def merged_by_sort(lists: np.ndarray) -> np.ndarray:
    n_lists, nq, k = lists.shape
    out = np.zeros((nq, k), dtype=np.uint64)
    for q in range(nq):
        if (lists[:, q, 0] == FAILED).any():
            out[q] = FAILED
            continue
        union = lists[:, q, :].reshape(-1)
        best = np.sort(union[union != 0])[::-1][:k]
        out[q, : len(best)] = best
    return out


MERGE_SHAPES = [(n, k) for k in (1, 256, 257, 1000, 16384) for n in (1, 2, 3, 8, 33, 64)]


@pytest.mark.parametrize("n_lists,k", MERGE_SHAPES)
def test_host_merge_of_long_lists_equals_a_sort_of_the_union(n_lists, k):
    rng = np.random.default_rng(1000 * n_lists + k)
    for nq, fill in ((1, "full"), (3, "ragged"), (2, "empty")):
        if k == 16384 and n_lists > 8 and fill != "full":
            continue  # (a million keys per query once is enough)
        lists = make_lists(rng, n_lists, nq, k, fill)
        got = _native.merge_topk_keys(lists)
        assert got.dtype == np.uint64 and got.shape == (nq, k)
        np.testing.assert_array_equal(got, merged_by_sort(lists))


def test_host_merge_more_lists_than_k_and_a_single_list():
    rng = np.random.default_rng(7)
    for n_lists, k in ((64, 1), (64, 5), (40, 7)):  # more lists than k
        lists = make_lists(rng, n_lists, 4, k, "ragged")
        np.testing.assert_array_equal(_native.merge_topk_keys(lists), merged_by_sort(lists))
    one = make_lists(rng, 1, 3, 1000, "ragged")  # one list: the merge is a copy
    np.testing.assert_array_equal(_native.merge_topk_keys(one), one[0])


@pytest.mark.parametrize("k", [1, 300, 16384])
def test_host_merge_a_list_leading_with_the_failure_key_fails_the_query_and_only_it(k):
    rng = np.random.default_rng(k)
    lists = make_lists(rng, 3, 4, k, "full")
    lists[1, 2, :] = FAILED  # rank 1 failed: TAVB_KEY_PEER_FAILED in every slot of its lists -- here for query 2
    lists[0, 3, 0] = FAILED  # and a list that merely LEADS with it
    got = _native.merge_topk_keys(lists)
    np.testing.assert_array_equal(got, merged_by_sort(lists))
    assert (got[2] == FAILED).all() and got[3, 0] == FAILED and (got[:2] != FAILED).all()
    with pytest.raises(_native.TavbError, match="a rank of the collective lookup failed"):
        _native.decode_keys(got)
    # two failed ranks: duplicated failure keys
    lists[2, 2, :] = FAILED
    assert (_native.merge_topk_keys(lists)[2] == FAILED).all()


def test_host_merge_refuses_bad_shapes():
    ok = np.zeros((2, 1, 4), dtype=np.uint64)
    out = np.zeros((1, 4), dtype=np.uint64)
    lib = _native.load_library(preload_torch=False)
    assert lib.tavb_merge_topk_host(_native._addr(ok), 2, 1, 4, _native._addr(out)) == 0
    for n_lists, nq, k in ((0, 1, 4), (65, 1, 4), (2, -1, 4), (2, 1, 0), (2, 1, _native.MAX_LARGE_K + 1)):
        assert lib.tavb_merge_topk_host(_native._addr(ok), n_lists, nq, k, _native._addr(out)) == -1
    assert lib.tavb_merge_topk_host(None, 2, 1, 4, _native._addr(out)) == -1
    assert lib.tavb_merge_topk_host(_native._addr(ok), 2, 0, 4, None) == 0  # no query: nothing to do
    assert lib.tavb_version() == 7  # additive: the ABI version stays


# ---- the SPMD form over gloo, with a numpy backend ----------------------------------------------------------------------------------

class NumpyShardBackend:
    """ShardBackend whose local search is the oracle over this rank's rows and whose merge is libtavb's host merge of long lists.
    TEST ONLY."""

    def __init__(self, shard: np.ndarray, row_offset: int, fail: bool = False):
        self.shard, self.row_offset, self.fail = shard, int(row_offset), fail

    @staticmethod
    def _keys(scores: np.ndarray, ids: np.ndarray, k: int) -> np.ndarray:
        keys = (scores.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids.astype(np.uint64))
        out = np.zeros(k, dtype=np.uint64)
        best = np.sort(keys)[::-1][:k]
        out[: len(best)] = best
        return out

    def _local(self, rows: np.ndarray, ids: np.ndarray, query: np.ndarray, k: int, thr: float) -> np.ndarray:
        from oracle import vectorbase_oracle as vo

        if self.fail:
            raise RuntimeError("injected failure of the local search")
        if len(rows) == 0:
            return np.zeros(k, dtype=np.uint64)
        sc = vo.scores_full(rows, query)
        keep = np.flatnonzero(sc >= np.float32(thr))
        return self._keys(sc[keep], np.asarray(ids)[keep], k)

    def local_search(self, queries, k, thr):
        q = queries.numpy()
        ids = np.arange(len(self.shard), dtype=np.int64) + self.row_offset
        return torch.from_numpy(np.stack([self._local(self.shard, ids, q[i], k, thr) for i in range(len(q))]).view(np.int64))

    def local_search_subset(self, query, local_rows, positions, k, thr):
        rows = self.shard[np.asarray(local_rows, dtype=np.int64)] if len(local_rows) else self.shard[:0]
        return torch.from_numpy(self._local(rows, np.asarray(positions), query, k, thr)[None, :].view(np.int64))

    def merge(self, gathered):
        return torch.from_numpy(_native.merge_topk_keys(gathered.numpy().view(np.uint64)).view(np.int64))

    def to_host(self, keys):
        return keys.numpy()

    def empty_gather(self, world, nq, k):
        return torch.empty((world, nq, k), dtype=torch.int64)

    def failed_lists(self, nq, k):
        return torch.full((nq, k), -1, dtype=torch.int64)

    def keys_to_device(self, keys):
        return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64))


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


TOTAL_ROWS, DIM = 2503, 48


def _worker(rank: int, world: int, port: int, fail_rank: int, ret):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import vectorbase_oracle as vo
        from tests.synth import make_corpus, make_queries
        from typeagent_py_amd.sharded import PeerFailedError, ShardedVectorBase, shard_range

        v, _ = make_corpus(TOTAL_ROWS, DIM, 777)
        qs = make_queries(3, DIM, 778)
        lo, hi = shard_range(TOTAL_ROWS, world, rank)
        backend = NumpyShardBackend(v[lo:hi], lo)
        svb = ShardedVectorBase(backend, lo, hi - lo, TOTAL_ROWS)
        rng = np.random.default_rng(9)
        subset = rng.integers(-5, TOTAL_ROWS, size=1800).tolist() + [0, 0, -1]
        sub_a = np.asarray(subset, dtype=np.int64)
        answers = {}
        for k in (300, 1000):
            for ms in (0.0, 0.5):
                hits = svb.fuzzy_lookup_embedding(qs[0], max_hits=k, min_score=ms)
                want = vo.lookup(v, qs[0], k, ms)
                assert len(hits) == len(want) and (ms > 0.0 or len(hits) == k)
                vo.check_topk_parity(vo.scores_full(v, qs[0]), [h.item for h in hits], [h.score for h in hits], k, ms)
                answers[(k, ms)] = [(h.item, h.score) for h in hits]
            batch = svb.fuzzy_lookup_embeddings(qs, max_hits=k, min_score=0.0)
            assert len(batch) == len(qs)
            for qi in range(len(qs)):
                assert len(batch[qi]) == k
                vo.check_topk_parity(vo.scores_full(v, qs[qi]), [h.item for h in batch[qi]], [h.score for h in batch[qi]], k, 0.0)
            got = svb.fuzzy_lookup_embedding_in_subset(qs[1], subset, max_hits=k, min_score=0.0)
            want = vo.lookup_in_subset(v, qs[1], subset, k, 0.0)
            assert len(got) == len(want) == k
            vo.check_topk_parity(vo.scores_full(v, qs[1])[sub_a], [h.item for h in got], [h.score for h in got], k, 0.0, candidate_ordinals=sub_a)
            row_to_msg = [i // 2 for i in range(TOTAL_ROWS)]
            msgs = svb.lookup_messages_by_embedding(qs[2], row_to_msg, max_matches=k, threshold_score=0.0)
            assert 0 < len(msgs) <= k and len({m.item for m in msgs}) == len(msgs)
        # what has no bounded per-rank list still raises, on every rank alike and before anything collective
        for bad in (0, 20000):
            with pytest.raises(ValueError, match="1..16384"):
                svb.fuzzy_lookup_embedding(qs[0], max_hits=bad)
            with pytest.raises(ValueError, match="1..16384"):
                svb.fuzzy_lookup_embeddings(qs, max_hits=bad)
            with pytest.raises(ValueError, match="1..16384"):
                svb.fuzzy_lookup_embedding_in_subset(qs[0], subset, max_hits=bad)
        with pytest.raises(ValueError):  # the predicate form keeps its limit
            svb.fuzzy_lookup_embedding(qs[0], max_hits=300, predicate=lambda i: True)

        # a failing rank: its own error there, PeerFailedError on every other rank, and the next collective lines up
        def outcome_of(call):
            try:
                call()
                return "answer"
            except PeerFailedError:
                return "peer"
            except RuntimeError as exc:
                return "own" if "injected failure" in str(exc) else f"other: {exc}"

        backend.fail = rank == fail_rank
        o_plain = outcome_of(lambda: svb.fuzzy_lookup_embedding(qs[0], max_hits=1000))
        o_sub = outcome_of(lambda: svb.fuzzy_lookup_embedding_in_subset(qs[1], subset, max_hits=300))
        backend.fail = False
        again = svb.fuzzy_lookup_embedding(qs[0], max_hits=1000, min_score=0.0)
        ret[rank] = (answers, o_plain, o_sub, [(h.item, h.score) for h in again] == answers[(1000, 0.0)])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_vectorbase_large_k_over_gloo_equals_the_whole_corpus(world):
    mgr = mp.Manager()
    ret = mgr.dict()
    fail_rank = 1
    mp.spawn(_worker, args=(world, _free_port(), fail_rank, ret), nprocs=world, join=True)
    assert set(ret.keys()) == set(range(world))
    for r in range(world):
        answers, o_plain, o_sub, lined_up = ret[r]
        assert answers == ret[0][0]  # every rank holds the same whole-corpus answer
        assert o_plain == o_sub == ("own" if r == fail_rank else "peer")
        assert lined_up
