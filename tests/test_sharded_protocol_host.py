"""CPU suite: the one exchange and the one failure protocol of `typeagent_py_amd/sharded.py`, through every lookup form of
`ShardedVectorBase` -- plain batch, subset, predicate, masked, top messages -- on one rank with a numpy backend of this file's own.

Per form and key family (k = 4: the fused family, k = 300: the large-k family; the predicate form keeps its limit of 256 and runs at 4):
  * `gather_fn = local[None]`: the answer of the same index without an exchange;
  * `gather_fn` that stacks a peer of failure lists: `PeerFailedError`;
  * a local part that raises, under either `gather_fn`: the injected error, AFTER `gather_fn` was called exactly once, with failure
    lists of shape [nq, k];
  * a local part that raises with no `gather_fn`, one rank and no communicator: the injected error at once, nothing exchanged.
Plus a mask that leaves this rank's part empty: the rank still joins, with zero lists."""

import numpy as np
import pytest
import torch

from oracle import vectorbase_oracle as vo
from tests import top_messages_shards_cases as tc
from tests.synth import make_corpus, make_queries
from tests.test_masked_shards_host import MaskedNumpyBackend
from typeagent_py_amd.sharded import PeerFailedError, ShardedVectorBase

N, D, NQ = 97, 16, 3
THR = 0.3
INJECTED = "injected failure of the local search"


class ProtocolBackend(MaskedNumpyBackend):
    """MaskedNumpyBackend + `local_survivors` and the top-messages local part, all of which raise while `fail` is set.  TEST ONLY."""

    def local_survivors(self, query, thr):
        if self.fail:
            raise RuntimeError(INJECTED)
        sc = vo.scores_full(self.shard, query)
        keep = np.flatnonzero(sc >= np.float32(thr))
        return keep.astype(np.int64) + self.row_offset, sc[keep]

    def set_row_messages(self, local_map, n_messages):
        self.local_map = np.asarray(local_map, dtype=np.int64)

    def local_top_messages(self, queries, k, thrs, handle=None, masked=False):
        if self.fail:
            raise RuntimeError(INJECTED)
        keys = np.zeros((len(queries), k), dtype=np.uint64)
        if not (masked and handle is None) and len(self.shard):
            allowed = None
            if masked:
                allowed = np.zeros(len(self.shard), dtype=bool)
                allowed[handle] = True
            for i, q in enumerate(queries):
                keys[i] = tc.collapse_keys(vo.scores_full(self.shard, q), self.local_map, k, thrs[i], allowed)
        return torch.from_numpy(keys.view(np.int64))


class Gather:
    """A `gather_fn` that records what it was handed.  peer_failed: stacks a second rank's lists, all of them failure lists."""

    def __init__(self, peer_failed: bool):
        self.peer_failed = peer_failed
        self.calls: list = []

    def __call__(self, local):
        self.calls.append(local.numpy().copy())
        return torch.stack([local, torch.full_like(local, -1)]) if self.peer_failed else local[None]


@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 5100)
    return v, make_queries(NQ, D, 5101)


def index(v, local_rows=N):
    backend = ProtocolBackend(v[:local_rows], 0)
    svb = ShardedVectorBase(backend, 0, local_rows, N)
    svb.set_row_messages(tc.message_map(N, "chunks3"))
    return svb, backend


MASK = np.random.default_rng(5102).random(N) < 0.5
SUBSET = np.random.default_rng(5103).integers(-3, N, size=40).tolist() + [0, 0]

# form -> (the call: (svb, queries, k) -> list of lists, the number of lists one exchange carries)
FORMS = {
    "plain": (lambda svb, qs, k: svb.fuzzy_lookup_embeddings(qs, k, THR), NQ),
    "subset": (lambda svb, qs, k: [svb.fuzzy_lookup_embedding_in_subset(qs[0], SUBSET, k, THR)], 1),
    "predicate": (lambda svb, qs, k: [svb.fuzzy_lookup_embedding(qs[0], k, THR, predicate=lambda i: i % 3 != 1)], 1),
    "masked": (lambda svb, qs, k: svb.fuzzy_lookup_embeddings_masked(qs, MASK, k, [0.0, THR, 0.5]), NQ),
    "top_messages": (lambda svb, qs, k: svb.lookup_top_messages_by_embeddings(qs, k, [0.0, THR, 0.5]), NQ),
    "top_messages_masked": (lambda svb, qs, k: svb.lookup_top_messages_by_embeddings(qs, k, THR, allowed=MASK), NQ),
}
CASES = [(form, k) for form in FORMS for k in (4, 300) if not (form == "predicate" and k == 300)]


@pytest.mark.parametrize("form,k", CASES)
def test_every_form_goes_through_one_exchange_and_one_failure_protocol(corpus, form, k):
    v, qs = corpus
    call, nq = FORMS[form]
    svb, backend = index(v)
    want = call(svb, qs, k)  # one rank, no gather_fn, no communicator: no exchange
    assert len(want) == nq and any(len(hits) for hits in want)

    for peer_failed in (False, True):
        gather = svb.searcher.gather_fn = Gather(peer_failed)
        if peer_failed:
            with pytest.raises(PeerFailedError, match="a rank of the collective lookup failed"):
                call(svb, qs, k)
        else:
            assert call(svb, qs, k) == want
        assert len(gather.calls) == 1 and gather.calls[0].shape == (nq, k) and (gather.calls[0] != -1).all()
        # a local part that raises: the failure lists travel first, then the rank's own error
        gather.calls.clear()
        backend.fail = True
        with pytest.raises(RuntimeError, match=INJECTED) as caught:
            call(svb, qs, k)
        backend.fail = False
        assert not isinstance(caught.value, PeerFailedError)
        assert len(gather.calls) == 1 and gather.calls[0].shape == (nq, k) and (gather.calls[0] == -1).all()

    # no gather_fn, one rank, no communicator: the error at once, nothing exchanged
    svb.searcher.gather_fn = None
    assert not svb.searcher.collective
    exchanged = []
    svb.searcher.exchange = lambda keys, messages=False: exchanged.append(tuple(keys.shape))
    backend.fail = True
    with pytest.raises(RuntimeError, match=INJECTED):
        call(svb, qs, k)
    assert exchanged == []


@pytest.mark.parametrize("form", ["masked", "top_messages_masked"])
@pytest.mark.parametrize("k", [4, 300])
def test_a_rank_whose_part_of_the_mask_is_empty_still_joins_with_zero_lists(corpus, form, k):
    v, qs = corpus
    svb, backend = index(v, local_rows=60)  # as rank 0 of two would hold it
    mask = np.zeros(N, dtype=bool)
    mask[70:80] = True  # allowed rows only in the other rank's part
    call = {"masked": lambda: svb.fuzzy_lookup_embeddings_masked(qs, mask, k, THR),
            "top_messages_masked": lambda: svb.lookup_top_messages_by_embeddings(qs, k, THR, allowed=mask)}[form]
    want = call()
    assert want == [[] for _ in range(NQ)]  # (this rank's part of the answer: nothing)
    gather = svb.searcher.gather_fn = Gather(False)
    assert call() == want
    assert len(gather.calls) == 1 and gather.calls[0].shape == (NQ, k) and (gather.calls[0] == 0).all()
    svb.searcher.gather_fn = Gather(True)
    with pytest.raises(PeerFailedError):
        call()


def test_the_collective_rule_is_one_property():
    v, _ = make_corpus(N, D, 5100)
    svb, backend = index(v)
    s = svb.searcher
    assert not s.collective and not s.native
    s.gather_fn = Gather(False)
    assert s.collective and not s.native
    backend.native_comm = True  # a communicator of the library: collective even on one rank; gather_fn still carries the exchange
    assert s.collective and not s.native
    s.gather_fn = None
    assert s.collective and s.native
    backend.native_comm = False
    s.always_collective = True  # only under an initialised torch.distributed
    assert not s.collective
