"""One device submission for all VectorBase lookups of one user question.

What the reference does per `ConversationBase.query()` (/root/reference):
  * T related-term lookups, sequential, each `fuzzy_lookup(term, max_hits=50, min_score=0.85)` on the
    terms corpus (storage/memory/reltermsindex.py:183-192 -> :320-332; settings convsettings.py:61-63);
  * one message re-rank: `lookup_in_subset_by_embedding` on the message-chunk corpus, a true subset
    gather in the memory provider (knowpro/textlocindex.py:164-177 -> vectorbase.py:203-230) or a full
    scan in the sqlite provider (storage/sqlite/messageindex.py:296-326), k = max_message_matches = 25
    (conversation_base.py:570), threshold 0.7 (convsettings.py:65-66);
  * zero or one thread lookup (storage/memory/convthreads.py:27-44), top-10 at the message-text
    threshold 0.7 (storage/memory/provider.py:64-65).
That is up to T + 2 synchronous numpy passes.  Here the T + 2 query vectors go to the GPU in one
copy, every scan is launched asynchronously on one stream (the T term queries share ONE pass over the
terms corpus), all result keys land in one buffer, and there is one device-to-host copy and one
stream synchronisation.  Results are identical to the separate calls (tests/test_gpu_parity.py).

BASELINE.json config 5 ("fused multi-index query") is defined on top of this class (bench.py
--workload cfg5), because the reference's tools/benchmark_query.py does not touch VectorBase at all
(correction 2).
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import _native
from .vectorbase import ScoredInt


@dataclass
class FusedResult:
    terms: list[list[ScoredInt]]  # one list per term query
    messages: list[ScoredInt]  # ordinals of the message corpus (subset: the caller's ordinals)
    threads: list[ScoredInt]


class FusedIndexQuery:
    """Holds up to three corpora (device tensors) behind one engine / one stream."""

    TERMS_K, TERMS_MIN = 50, 0.85
    MESSAGES_K, MESSAGES_MIN = 25, 0.7
    THREADS_K, THREADS_MIN = 10, 0.7

    def __init__(self, device: int = 0):
        import torch

        self.torch = torch
        self.device = int(device)
        torch.cuda.set_device(self.device)
        self.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.stream):
            self.engine = _native.Engine(self.device, use_torch_stream=True)
        self.corpora: dict[str, tuple] = {}
        self._pinned_q = None
        self._dev_q = None
        self._pinned_keys = None
        self._shape = None  # (nq, dim, TERMS_K, MESSAGES_K, THREADS_K) the buffers and views above were made for

    def set_corpus(self, name: str, tensor, rows: int | None = None) -> None:
        """name in {"terms", "messages", "threads"}; tensor: contiguous f32/f16 [N, D] on this device."""
        if name not in ("terms", "messages", "threads"):
            raise ValueError("corpus name must be terms, messages or threads")
        n = tensor.shape[0] if rows is None else int(rows)
        self.corpora[name] = (tensor, n)

    def _has(self, name: str) -> bool:
        entry = self.corpora.get(name)
        return entry is not None and entry[1] > 0

    def _use(self, name: str) -> bool:
        entry = self.corpora.get(name)
        if entry is None or entry[1] == 0:
            return False
        self.engine.set_corpus_tensor(entry[0], rows=entry[1], ordinal_base=0, sync_torch=False)
        return True

    def _alloc(self, nq: int, dim: int, n_keys: int):
        """(pinned f32 [nq, dim] queries, device f32 [nq, dim] queries, pinned int64 [n_keys] result keys) of one run shape."""
        torch = self.torch
        dev = torch.device("cuda", self.device)
        pinned_q = torch.empty((nq, dim), dtype=torch.float32).pin_memory()
        dev_q = torch.empty((nq, dim), dtype=torch.float32, device=dev)
        return pinned_q, dev_q, torch.zeros(n_keys, dtype=torch.int64).pin_memory()

    def run(self, term_queries, message_query=None, thread_query=None, message_subset=None) -> FusedResult:
        torch = self.torch
        tq = np.ascontiguousarray(term_queries, dtype=np.float32).reshape(-1, np.shape(term_queries)[-1]) if len(term_queries) else np.zeros((0, 0), np.float32)
        T = tq.shape[0]
        dim = tq.shape[1] if T else (len(message_query) if message_query is not None else len(thread_query))
        nq = T + 2
        tk, mk, hk = int(self.TERMS_K), int(self.MESSAGES_K), int(self.THREADS_K)
        # the subset is checked before anything is enqueued: an error raised after the H2D copy of the queries would leave that copy reading
        # the pinned query buffer the next run() writes
        subset = rows = None
        if message_query is not None and message_subset is not None and self._has("messages"):
            subset = np.asarray(message_subset, dtype=np.int64).reshape(-1)
            n = self.corpora["messages"][1]
            rows = np.where(subset < 0, subset + n, subset)
            if ((rows < 0) | (rows >= n)).any():
                raise IndexError("message subset ordinal out of range")
        shape = (nq, dim, tk, mk, hk)
        if self._shape != shape:
            # the result keys land in pinned host memory straight from the last kernel of every lookup (no device buffer, no copy back, no
            # memset launch in front: at the reference's scale a user query is launch-bound -- ten submissions were 98 us, profiles/r06_raw/
            # cfg5_reference_scale.txt); the views handed to the engine are made once per shape (a tensor slice costs 2-3 us of host time).
            # Each lookup gets a contiguous block of its own k per query -- [T, TERMS_K], [1, MESSAGES_K], [1, THREADS_K] -- because the
            # kernels write row q of a lookup at q * k: a slice of a wider buffer would be strided, and a cache kept across a change of the
            # K attributes would be too small.
            self._pinned_q, self._dev_q, self._pinned_keys = self._alloc(nq, dim, T * tk + mk + hk)
            keys = self._pinned_keys
            self._keys_np = keys.numpy()
            self._host_q = self._pinned_q.numpy()
            self._views = {
                "tq": self._dev_q[:T], "tk": keys[: T * tk].view(T, tk),
                "mq": self._dev_q[T : T + 1], "mq1": self._dev_q[T], "mk": keys[T * tk : T * tk + mk].view(1, mk),
                "hq": self._dev_q[T + 1 : T + 2], "hk": keys[T * tk + mk :].view(1, hk),
            }
            self._shape = shape
        host_q, views, keys_np = self._host_q, self._views, self._keys_np
        if T:
            host_q[:T] = tq
        host_q[T] = 0 if message_query is None else np.asarray(message_query, dtype=np.float32)
        host_q[T + 1] = 0 if thread_query is None else np.asarray(thread_query, dtype=np.float32)
        thr = _native.f32_threshold
        ran_t = ran_m = ran_h = False
        with torch.cuda.stream(self.stream):
            self._dev_q.copy_(self._pinned_q, non_blocking=True)
            if T and self._use("terms"):
                self.engine.search_device(views["tq"], tk, float(thr(self.TERMS_MIN)), out_keys=views["tk"])
                ran_t = True
            if message_query is not None and self._use("messages"):
                if subset is not None:
                    if len(rows):
                        d_rows = torch.from_numpy(rows.astype(np.int32)).to(self._dev_q.device, non_blocking=True)
                        self.engine.search_subset_device(views["mq1"], d_rows, mk, float(thr(self.MESSAGES_MIN)), out_keys=views["mk"])
                        ran_m = True
                else:
                    self.engine.search_device(views["mq"], mk, float(thr(self.MESSAGES_MIN)), out_keys=views["mk"])
                    ran_m = True
            if thread_query is not None and self._use("threads"):
                self.engine.search_device(views["hq"], hk, float(thr(self.THREADS_MIN)), out_keys=views["hk"])
                ran_h = True
        self.stream.synchronize()
        # (a lookup that did not run leaves last call's keys in its block: empty it; the others were overwritten in full by their merge kernels)
        t_keys, m_keys, h_keys = keys_np[: T * tk].reshape(T, tk), keys_np[T * tk : T * tk + mk].reshape(1, mk), keys_np[T * tk + mk :].reshape(1, hk)
        if T and not ran_t:
            t_keys[:] = 0
        if not ran_m:
            m_keys[:] = 0
        if not ran_h:
            h_keys[:] = 0

        def hits(block, row: int = 0, remap=None) -> list[ScoredInt]:
            ords, scs, cnts = block
            m = int(cnts[row])
            items = ords[row, :m].tolist()
            if remap is not None:
                items = [int(remap[i]) for i in items]
            return [ScoredInt(int(i), float(s)) for i, s in zip(items, scs[row, :m].tolist())]

        terms = _native.decode_keys(t_keys) if T else None
        return FusedResult([hits(terms, i) for i in range(T)], hits(_native.decode_keys(m_keys), 0, subset), hits(_native.decode_keys(h_keys)))
