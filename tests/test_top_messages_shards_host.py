"""CPU suite: top-k distinct messages on device groups and row-sharded indexes.

  * `tavb_merge_top_messages_host` (`_native.merge_top_messages_keys`) against the numpy statement of the merge: lists in which one message
    stands several times, full, ragged and empty, a failed list among real ones;
  * "every shard's own top K, then the merge" equals the collapse over the whole corpus, restated in numpy;
  * `ShardedVectorBase` over gloo with world 2 and 3 and a numpy backend of this file's own: unmasked and masked top-messages lookups equal
    the whole-corpus collapse, a failing rank raises on itself and `PeerFailedError` everywhere else, max_messages 0 and 20000 raise.

No GPU: the host merge is a pure host helper of libtavb.so, and the backend's local part is the oracle."""

import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import top_messages_shards_cases as tc
from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", [1, 10, 257, 16384])
@pytest.mark.parametrize("n_lists", [1, 2, 3, 8, 64])
def test_host_merge_of_top_messages_lists_equals_the_numpy_statement(n_lists, k):
    rng = np.random.default_rng(1000 * n_lists + k)
    for nq, fill in ((1, "full"), (3, "ragged"), (2, "empty")):
        if k == 16384 and n_lists > 8 and fill != "full":
            continue  # (a million keys per query once is enough)
        for n_messages in (max(k // 2, 1), 3 * k):  # fewer distinct messages than k, and more
            lists = tc.random_lists(rng, n_lists, nq, k, fill, n_messages)
            got = _native.merge_top_messages_keys(lists)
            assert got.dtype == np.uint64 and got.shape == (nq, k)
            np.testing.assert_array_equal(got, tc.merge_statement(lists))


def test_host_merge_duplicates_one_entry_per_message():
    k, n_lists = 10, 4
    msgs = np.arange(25)
    rng = np.random.default_rng(3)
    lists = np.zeros((n_lists, 1, k), dtype=np.uint64)
    scores = rng.random((n_lists, len(msgs))).astype(np.float32)
    for l in range(n_lists):  # every list holds the same messages, with different scores
        lists[l, 0] = np.sort(tc.make_keys(scores[l], msgs))[::-1][:k]
    got = _native.merge_top_messages_keys(lists)
    np.testing.assert_array_equal(got, tc.merge_statement(lists))
    ords, _ = tc.decoded(got[0])
    assert len(ords) == k == len(set(ords))
    same = np.repeat(lists[:1], 3, axis=0)  # the same key in every list gives one entry
    np.testing.assert_array_equal(_native.merge_top_messages_keys(same), lists[0])
    few = np.zeros((3, 1, k), dtype=np.uint64)  # fewer distinct messages than k: zero-padded
    for l in range(3):
        few[l, 0, :4] = np.sort(tc.make_keys([0.5 + 0.1 * l, 0.2, 0.9 - 0.2 * l, 0.0], [7, 8, 9, 11]))[::-1]
    got = _native.merge_top_messages_keys(few)
    np.testing.assert_array_equal(got, tc.merge_statement(few))
    assert tc.decoded(got[0])[0] == [9, 7, 8, 11] and (got[0, 4:] == 0).all()


@pytest.mark.parametrize("k", [1, 300, 16384])
def test_host_merge_a_failed_list_fails_the_query_and_only_it(k):
    rng = np.random.default_rng(k)
    lists = tc.random_lists(rng, 3, 4, k, "full", 2 * k)
    lists[1, 2, :] = tc.FAILED
    lists[0, 3, 0] = tc.FAILED
    got = _native.merge_top_messages_keys(lists)
    np.testing.assert_array_equal(got, tc.merge_statement(lists))
    assert (got[2:] == tc.FAILED).all() and (got[:2] != tc.FAILED).all()
    with pytest.raises(_native.TavbError, match="a rank of the collective lookup failed"):
        _native.decode_keys(got)


def test_host_merge_refuses_bad_shapes():
    ok = np.zeros((2, 1, 4), dtype=np.uint64)
    out = np.zeros((1, 4), dtype=np.uint64)
    lib = _native.load_library(preload_torch=False)
    assert lib.tavb_merge_top_messages_host(_native._addr(ok), 2, 1, 4, _native._addr(out)) == 0
    for n_lists, nq, k in ((0, 1, 4), (65, 1, 4), (2, -1, 4), (2, 1, 0), (2, 1, _native.MAX_LARGE_K + 1)):
        assert lib.tavb_merge_top_messages_host(_native._addr(ok), n_lists, nq, k, _native._addr(out)) == -1
    assert lib.tavb_merge_top_messages_host(None, 2, 1, 4, _native._addr(out)) == -1
    assert lib.tavb_merge_top_messages_host(_native._addr(ok), 2, 0, 4, None) == 0
    assert lib.tavb_version() == 7  # additive: the ABI version stays
    for name in ("tavb_merge_top_messages_device", "tavb_search_top_messages_allgather", "tavb_allgather_merge_top_messages"):
        assert name in _native.ABI_SYMBOLS and getattr(lib, name)


# ---- every shard's own top K, then the merge == the collapse over the whole corpus ------------------------------------------------------

ROWS, BOUNDS = 2000, [0, 667, 1334, 2000]  # (667 and 1334 are no multiples of 3: messages of 3 chunks straddle both)


@pytest.mark.parametrize("kind", ["chunks3", "interleaved", "interleaved_holes", "all_equal"])
def test_per_shard_top_k_then_merge_equals_the_whole_corpus_collapse(kind):
    rng = np.random.default_rng(17)
    mapping = tc.message_map(ROWS, "chunks3" if kind == "all_equal" else kind)
    n_messages = int(mapping.max()) + 1
    for trial in range(3):
        scores = np.full(ROWS, 0.75, np.float32) if kind == "all_equal" else rng.choice(np.linspace(0, 1, 61, dtype=np.float32), size=ROWS)
        allowed = None if trial == 0 else rng.random(ROWS) < (0.5 if trial == 1 else 0.02)
        for k in (1, 10, 300, n_messages + 5):
            for thr in (0.0, 0.5, 1.5):
                want = tc.collapse_keys(scores, mapping, k, thr, allowed)
                got = tc.shard_then_merge(scores, mapping, k, thr, BOUNDS, allowed)
                np.testing.assert_array_equal(got, want, err_msg=f"{kind} trial={trial} k={k} thr={thr}")
                if kind == "all_equal" and thr <= 0.75 and allowed is None:
                    assert tc.decoded(want)[0] == list(range(min(k, n_messages)))  # ties: ascending message ordinal


# ---- the SPMD form over gloo, with a numpy backend ----------------------------------------------------------------------------------

def row_scores(rows: np.ndarray, query: np.ndarray) -> np.ndarray:
    """The public score of every row, each row summed on its own: a row scores the same in a shard as in the whole corpus, bit for bit
    (a BLAS product over another number of rows may block its sums differently)."""
    from oracle import vectorbase_oracle as vo

    return vo.cosine_to_score(np.sum(rows * query[None, :], axis=1, dtype=np.float32))


class NumpyMessagesBackend:
    """ShardBackend with no top-messages methods of its own: `local_survivors` is the oracle over this rank's rows.  TEST ONLY."""

    def __init__(self, shard: np.ndarray, row_offset: int):
        self.shard, self.row_offset, self.fail = shard, int(row_offset), False

    def local_survivors(self, query, thr):
        if self.fail:
            raise RuntimeError("injected failure of the local search")
        sc = row_scores(self.shard, query)
        keep = np.flatnonzero(sc >= np.float32(thr))
        return keep.astype(np.int64) + self.row_offset, sc[keep]

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
        from tests.synth import make_corpus, make_queries
        from typeagent_py_amd.sharded import PeerFailedError, ShardedVectorBase, shard_range

        v, _ = make_corpus(TOTAL_ROWS, DIM, 777)
        qs = make_queries(3, DIM, 778)
        lo, hi = shard_range(TOTAL_ROWS, world, rank)
        backend = NumpyMessagesBackend(v[lo:hi], lo)
        svb = ShardedVectorBase(backend, lo, hi - lo, TOTAL_ROWS)
        with pytest.raises(RuntimeError, match="set_row_messages"):
            svb.lookup_top_messages_by_embeddings(qs)
        mask = np.random.default_rng(5).random(TOTAL_ROWS) < 0.3
        upper = mask.copy()
        upper[: hi if rank == 0 else shard_range(TOTAL_ROWS, world, 0)[1]] = False  # nothing allowed in rank 0's part
        answers = {}
        for kind in ("chunks3", "interleaved"):
            mapping = tc.message_map(TOTAL_ROWS, kind)
            svb.set_row_messages(mapping)
            for name, allowed in (("none", None), ("mask", mask), ("upper", upper)):
                handle = None if allowed is None else svb.row_mask(allowed)
                for k in (10, 1000):
                    thrs = [0.0, 0.5, 0.0]
                    got = svb.lookup_top_messages_by_embeddings(qs, k, thrs, allowed=handle)
                    for i in range(3):
                        want = tc.collapse_keys(row_scores(v, qs[i]), mapping, k, thrs[i], allowed)
                        assert ([h.item for h in got[i]], np.asarray([h.score for h in got[i]], np.float32).view(np.uint32).tolist()) == tc.decoded(want)
                    one = svb.lookup_top_messages_by_embedding(qs[1], k, 0.5, allowed=handle)
                    assert one == got[1]
                    answers[(kind, name, k)] = [[(h.item, h.score) for h in hits] for hits in got]
        assert svb.lookup_top_messages_by_embeddings(qs, 10, 0.0, allowed=np.zeros(TOTAL_ROWS, bool)) == [[], [], []]  # no exchange: nobody waits
        assert svb.lookup_top_messages_by_embeddings(qs[:0], 10) == []
        for bad in (0, 20000):
            with pytest.raises(ValueError, match="1..16384"):
                svb.lookup_top_messages_by_embeddings(qs, max_messages=bad)
            with pytest.raises(ValueError, match="1..16384"):
                svb.lookup_top_messages_by_embedding(qs[0], max_messages=bad)

        def outcome_of(call):
            try:
                call()
                return "answer"
            except PeerFailedError:
                return "peer"
            except RuntimeError as exc:
                return "own" if "injected failure" in str(exc) else f"other: {exc}"

        backend.fail = rank == fail_rank
        o_plain = outcome_of(lambda: svb.lookup_top_messages_by_embeddings(qs, 10))
        o_mask = outcome_of(lambda: svb.lookup_top_messages_by_embeddings(qs, 300, allowed=mask))
        backend.fail = False
        again = svb.lookup_top_messages_by_embeddings(qs, 10, [0.0, 0.5, 0.0])
        ret[rank] = (answers, o_plain, o_mask, [[(h.item, h.score) for h in hits] for hits in again] == answers[("interleaved", "none", 10)])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_vectorbase_top_messages_over_gloo_equals_the_whole_corpus(world):
    mgr = mp.Manager()
    ret = mgr.dict()
    fail_rank = 1
    mp.spawn(_worker, args=(world, _free_port(), fail_rank, ret), nprocs=world, join=True)
    assert set(ret.keys()) == set(range(world))
    for r in range(world):
        answers, o_plain, o_mask, lined_up = ret[r]
        assert answers == ret[0][0]  # every rank holds the same whole-corpus answer
        assert o_plain == o_mask == ("own" if r == fail_rank else "peer")
        assert lined_up
