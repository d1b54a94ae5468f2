"""Row-sharded lookup across the GPUs of one node: one process per GPU
(`torch.distributed`, backend "nccl" == RCCL over xGMI), each rank owning a
contiguous range of corpus rows.

Why this shards: a row's score depends only on that row
and the query (vectorbase.py:176 of the reference), so the global top-k is the
top-k of the union of the per-shard top-k lists.  The only exchange step is an
all-gather of the per-rank packed result keys -- `nq * k * 8` bytes per rank
(256 KiB at nq=1024, k=32), latency-bound, far below xGMI link bandwidth --
followed by a local k-way merge kernel on every rank.  No all-reduce, no
tensor/pipeline parallelism: there is nothing else to exchange on this path.

Result keys are `(score bits << 32) | (0xFFFFFFFF - global_ordinal)`, so the
merge is a pure integer max-merge and ties resolve to the smaller global
ordinal on every rank identically (all ranks return the same answer).

The product backend (`DeviceShardBackend`) issues the exchange from inside
libtavb: `tavb_search_allgather` = scan kernels -> `ncclAllGather` (RCCL, on the
context's stream) -> merge kernel, written straight into pinned host memory.
`torch.distributed` is used ONCE, to hand rank 0's 128-byte RCCL rendezvous id to
the other ranks (`init_comm`); the lookup path does not touch it.

The compute backend is injected so that the communication pattern can be tested
on CPU with `gloo` (tests/test_sharded_gloo.py supplies a host backend: for such
backends the searcher falls back to `torch.distributed.all_gather_into_tensor`);
the product backend below is the only one this package ships and it runs the HIP
kernels.  There is no CPU fallback in the product path.

max_hits 257 .. 16384 take the same steps with the large-k calls of the library: `tavb_search_topk_allgather` (the exact device top-k of
the shard, the all-gather in chunks of whole queries, the merge of long lists), `tavb_search_topk_device` + `tavb_allgather_merge_topk`
for the subset form.  max_hits = 0 (every survivor) and max_hits above 16384 have no bounded list to exchange and raise ValueError here;
a `VectorBase(devices=[...])` device group serves them through its emit-all route.

Masked lookups: every rank expands ITS slice of the mask on its device once (`DeviceShardBackend.mask_to_device`, tavb_mask_expand), a
batch of queries is one `tavb_search_subset_batch_device` per rank -- keys carrying global ordinals -- and ONE exchange of the [nq, k] lists.

Top-k distinct messages (`set_row_messages`, `lookup_top_messages_by_embedding(s)`): every rank holds its slice of ONE global row -> message
map with the global message count, a batch is `tavb_search_top_messages_allgather` -- the rank's own best k messages, the all-gather, one
maximum per message and the best k of those -- and every rank returns the whole-corpus answer.

One copy of each step: `ShardedSearcher.collective` answers "does this call exchange", `ShardedSearcher.exchange` is the only exchange (the
library's communicator -> `gather_fn` -> a single rank -> torch.distributed) and `ShardedSearcher.lookup_keys` the only failure protocol
(the local part, failure lists in its place when it raises, the exchange, the rank's own error, `_raise_if_peer_failed`): every lookup
form of `ShardedVectorBase` hands it its local part.  The library's one-call paths run the protocol inside libtavb and share the last step.
"""

from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Protocol

import numpy as np

from . import _native


def shard_range(total_rows: int, world_size: int, rank: int) -> tuple[int, int]:
    """Contiguous row range [lo, hi) of `rank`: the first (total % world) ranks get one extra row."""
    base, extra = divmod(total_rows, world_size)
    lo = rank * base + min(rank, extra)
    hi = lo + base + (1 if rank < extra else 0)
    return lo, hi


class ShardBackend(Protocol):
    def local_search(self, queries, k: int, thr: float):  # -> tensor int64 [nq, k] packed keys (global ordinals)
        ...

    def merge(self, gathered):  # tensor int64 [world, nq, k] -> tensor int64 [nq, k]
        ...

    def to_host(self, keys) -> np.ndarray:  # -> int64 [nq, k]
        ...

    def empty_gather(self, world: int, nq: int, k: int):  # tensor int64 [world, nq, k] on the backend's device
        ...

    def failed_lists(self, nq: int, k: int):  # tensor int64 [nq, k] of PEER_FAILED_KEY, ordered in front of the exchange that follows
        ...

    # the forms beside the plain lookup (ShardedVectorBase: subset, predicate) -------------------------------------------------------
    def local_search_subset(self, query: np.ndarray, local_rows: np.ndarray, positions: np.ndarray, k: int, thr: float):  # -> tensor int64 [1, k], keys carrying `positions`
        ...

    def local_survivors(self, query: np.ndarray, thr: float):  # -> (global ordinals int64, scores float32) of every row of the shard with score >= thr
        ...

    def keys_to_device(self, keys: np.ndarray):  # uint64 / int64 [nq, k] host keys -> tensor on the backend's device
        ...

    # storage (ShardedVectorBase.add_embedding(s) / serialize / deserialize / clear) --------------------------------------------------
    def set_rows(self, rows: np.ndarray, row_offset: int, dtype: str = "fp32") -> None:  # replace this rank's shard (float32 [n, dim]; no rows: drop it)
        ...

    def append_rows(self, rows: np.ndarray) -> None:  # append float32 [n, dim] to this rank's shard
        ...

    def rows_to_host(self) -> np.ndarray:  # this rank's rows as float32 [n, dim]
        ...

    # Optional capabilities, probed with hasattr / getattr (test doubles leave them out on purpose) and what each unlocks:
    #   native_comm (attribute)                the library's own communicator: `search_allgather` serves the plain lookup in one C call and
    #                                          the engine's allgather_merge* calls serve every other exchange (unless `gather_fn` is set)
    #   stage_queries(q)                       host queries -> device through a reused pinned buffer (else a plain torch copy)
    #   subset_to_device(local_rows, positions) + local_search_subset_resident(query, handle, k, thr)
    #                                          this shard's part of a caller's subset stays on the device while the same list comes back
    #   mask_to_device(local_mask) + local_search_masked(queries, handle, k, thrs)
    #                                          masked batches as ONE local call and ONE exchange (else the subset lookup per query)
    #   local_top_messages(queries, k, thrs, handle, masked)
    #                                          this rank's best k messages on the device (else `local_survivors` and a collapse on the host)
    #   merge_top_messages(gathered)           the top-messages merge on the device (else libtavb's host merge)
    #   search_top_messages_allgather(...) + join_failed_top_messages(nq, k, n_messages)
    #                                          with native_comm: a top-messages batch in one C call
    #   set_row_messages(local_map, n_messages) this rank's slice of the row -> message map on its device
    #   storage_dtype()                        what `rebalance()` keeps the shard stored as
    #   stream, torch (attributes)             the stream the backend's kernels run on: the torch.distributed all-gather is issued on it


def _fused_k(k: int) -> bool:
    """the fused selection family of the library (k <= 256) or, False, its large-k family: the one place that decides from k"""
    return k <= _native.MAX_FUSED_K


def _pack_keys(scores: np.ndarray, ordinals: np.ndarray) -> np.ndarray:
    """(float32 scores, ordinals) -> uint64 result keys: (score bits << 32) | (0xFFFFFFFF - ordinal)"""
    return (scores.astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ordinals.astype(np.uint64))


def _check_k(k: int, what: str) -> None:
    if not (1 <= k <= _native.MAX_LARGE_K):
        raise ValueError(f"{what} must be in 1..{_native.MAX_LARGE_K} for a row-sharded lookup (0 = every survivor and larger values have no bounded "
                         "per-rank list to exchange: a VectorBase(devices=[...]) device group serves them)")


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def _popcount(words: np.ndarray) -> int:
    """set bits of a packed mask (uint32 words, tail bits zero)"""
    return int(_POP8[words.view(np.uint8)].sum(dtype=np.int64))


PEER_FAILED_KEY = -1  # TAVB_KEY_PEER_FAILED (all bits set) seen as int64: what a rank whose local search failed contributes to the exchange


class PeerFailedError(RuntimeError):
    """Another rank's local search failed during a collective lookup: the merged lists would be missing its shard."""


def _raise_if_peer_failed(keys: np.ndarray) -> np.ndarray:
    """merged host keys [nq, k] -> the same keys, unless a list leads with the failure key (it sorts above every real key, so a failed rank's
    contribution leads every merged list on every rank)"""
    if keys.size and (np.asarray(keys).reshape(keys.shape[0], -1)[:, 0].view(np.int64) == PEER_FAILED_KEY).any():
        raise PeerFailedError("a rank of the collective lookup failed in its local part: the merged lists are missing its shard")
    return keys


class DeviceShardBackend:
    """HIP kernels on this rank's GPU, launched on a dedicated torch stream so that
    RCCL collectives issued by torch.distributed order correctly with them."""

    def __init__(self, device: int):
        import torch

        self.torch = torch
        self.device = int(device)
        torch.cuda.set_device(self.device)
        self._dev = torch.device("cuda", self.device)
        self.stream = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.stream):
            self.engine = _native.Engine(self.device, use_torch_stream=True)
        self._pinned: dict = {}
        self._gather: dict = {}
        self._failed: dict = {}
        self._qstage: dict = {}
        self._dtype_name = "fp32"
        self.native_comm = False  # True once init_comm() has joined the library's own RCCL communicator

    def set_shard(self, tensor, row_offset: int, rows: int | None = None) -> None:
        self.engine.set_corpus_tensor(tensor, rows=rows, ordinal_base=row_offset)
        self._dtype_name = "fp16" if tensor.dtype == self.torch.float16 else "fp32"

    def storage_dtype(self) -> str:
        """"fp16" / "fp32": what this rank's shard is stored as (what `rebalance()` keeps)."""
        return self._dtype_name

    def stage_queries(self, q: np.ndarray):
        """host float32 [nq, dim] -> device tensor, through a reused pinned buffer on the backend's stream (no pageable staging copy per call)."""
        torch = self.torch
        shape = tuple(q.shape)
        slot = self._qstage.get(shape)
        if slot is None:
            if len(self._qstage) >= 8:
                self._qstage.clear()
            with torch.cuda.stream(self.stream):
                slot = self._qstage[shape] = (torch.empty(shape, dtype=torch.float32).pin_memory(), torch.empty(shape, dtype=torch.float32, device=self._dev))
        pinned, dev = slot
        self.stream.synchronize()  # (the previous lookup that read `dev` is long done in practice; cheap)
        pinned.numpy()[...] = q
        with torch.cuda.stream(self.stream):
            dev.copy_(pinned, non_blocking=True)
        return dev

    def init_comm(self, rank: int, world: int, exchange_id=None) -> None:
        """Collective: join libtavb's own RCCL communicator (tavb_comm_init).  Rank 0 creates the rendezvous id; `exchange_id(id or None)
        -> id` distributes it (default: `torch.distributed.broadcast_object_list` over the default group, whatever its backend)."""
        uid = _native.comm_unique_id() if rank == 0 else None
        if world > 1 or exchange_id is not None:
            if exchange_id is None:
                import torch.distributed as dist

                box = [uid]
                dist.broadcast_object_list(box, src=0)
                uid = box[0]
            else:
                uid = exchange_id(uid)
        with self.torch.cuda.stream(self.stream):
            self.engine.comm_init(uid, rank, world)
        self.native_comm = True

    # -- storage: this rank's rows (vectorbase.py:115-148, 268-287 over a row-sharded corpus) ------------------------------------------
    def set_rows(self, rows: np.ndarray, row_offset: int, dtype: str = "fp32") -> None:
        """Replace this rank's shard by host rows (float32 [n, dim]); uploaded through the pinned ring (tavb_upload_rows)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        self._dtype_code = _native.TAVB_F16 if dtype == "fp16" else _native.TAVB_F32
        self._dtype_name = "fp16" if dtype == "fp16" else "fp32"
        with self.torch.cuda.stream(self.stream):
            self.engine.ordinal_base = int(row_offset)
            if rows.ndim == 2 and rows.shape[1] > 0:
                self.engine.upload_rows(rows, 0, self._dtype_code, capacity_hint=2 * rows.shape[0])
            else:
                self.engine.clear()

    def append_rows(self, rows: np.ndarray) -> None:
        """Append host rows (float32 [n, dim]) to this rank's shard: only the new rows travel (capacity doubles; a shard adopted from the
        caller's tensor is copied into a buffer of the backend's own first)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        code = self.engine.dtype if self.engine.corpus is not None else getattr(self, "_dtype_code", _native.TAVB_F32)
        with self.torch.cuda.stream(self.stream):
            self.engine.upload_rows(rows, self.engine.rows if self.engine.corpus is not None else 0, code)

    def rows_to_host(self) -> np.ndarray:
        """This rank's rows as float32 [n, dim] (fp16 storage widened)."""
        self.stream.synchronize()
        if self.engine.corpus is None:
            return np.zeros((0, 0), dtype=np.float32)
        return self.engine.corpus[: self.engine.rows].float().cpu().numpy()

    # -- the forms beside the plain lookup: this shard's part, as keys that already carry GLOBAL positions / ordinals ----------------
    def local_search_subset(self, query: np.ndarray, local_rows: np.ndarray, positions: np.ndarray, k: int, thr: float):
        """rows of THIS shard (local numbering) that the caller's subset names, `positions[i]` = where local_rows[i] sits in the
        caller's list -> keys [1, k] carrying those positions (subset gather kernel + position remap, on the backend's stream)."""
        return self.local_search_subset_resident(query, self.subset_to_device(local_rows, positions), k, thr)

    def _zero_keys(self, nq: int, k: int):
        """[nq, k] zero keys on the backend's stream: what a rank contributes whose part of a subset, a mask or the corpus is empty"""
        with self.torch.cuda.stream(self.stream):
            return self.torch.zeros((nq, k), dtype=self.torch.int64, device=self._dev)

    def subset_to_device(self, local_rows: np.ndarray, positions: np.ndarray):
        """This shard's part of a caller's subset as device tensors (rows int32 [S], positions int32 [S]) -- a handle for
        `local_search_subset_resident`; None when no row of the subset lies in this shard."""
        torch = self.torch
        if len(local_rows) == 0:
            return None
        with torch.cuda.stream(self.stream):  # (the copies run on the backend's stream, in front of the kernels that read them)
            return (torch.from_numpy(np.ascontiguousarray(local_rows, dtype=np.int32)).to(self._dev),
                    torch.from_numpy(np.ascontiguousarray(positions, dtype=np.int32)).to(self._dev))

    def local_search_subset_resident(self, query: np.ndarray, handle, k: int, thr: float):
        """`local_search_subset` over a handle of `subset_to_device`: only the query travels.  The fused selection up to MAX_FUSED_K, the
        exact device top-k beyond; either gives keys carrying positions in this shard's part, remapped to the caller's positions."""
        if handle is None:
            return self._zero_keys(1, k)
        with self.torch.cuda.stream(self.stream):
            dq = self.torch.from_numpy(np.ascontiguousarray(query, dtype=np.float32)).to(self._dev)
            if _fused_k(k):
                keys = self.engine.search_subset_device(dq, handle[0], k, thr)
            else:
                keys = self.engine.search_topk_device(dq.reshape(1, -1), k, thr, dev_rows=handle[0])
            self.engine.remap_key_positions(keys, handle[1])
            self._keep = (dq, handle)  # alive until the next call (the kernels run asynchronously)
            return keys

    # -- masked lookups: this rank's slice of a mask, expanded once and kept on the device ------------------------------------------------
    def mask_to_device(self, local_mask):
        """This rank's slice of an allow-mask (numpy bool [local_rows], or a torch bool tensor on this device) -> the allowed local rows
        as a device tensor (int32, ascending; tavb_mask_expand) -- a handle for `local_search_masked`; None when the slice allows no row."""
        if len(local_mask) == 0:
            return None
        if hasattr(local_mask, "is_cuda"):
            # whatever produced a tensor mask ran on the CALLER's stream; inside the context below the current stream is the backend's own
            # (the engine's), so the synchronise of Engine.pack_mask_tensor would wait for the wrong one
            self.torch.cuda.current_stream(self.device).synchronize()
        with self.torch.cuda.stream(self.stream):
            dev_rows, count = self.engine.mask_to_rows(local_mask)
        return dev_rows if count else None

    def local_search_masked(self, queries: np.ndarray, handle, k: int, thrs):
        """A batch of queries (host float32 [nq, dim]; thrs: one threshold per query) over a handle of `mask_to_device`: ONE
        tavb_search_subset_batch_device on the backend's stream -> keys [nq, k] carrying GLOBAL ordinals (the engine's ordinal_base is this
        rank's row_offset).  Asynchronous; an empty part (handle None) gives zero keys."""
        if handle is None:
            return self._zero_keys(int(np.shape(queries)[0]), k)
        dq = self.stage_queries(np.ascontiguousarray(queries, dtype=np.float32))
        with self.torch.cuda.stream(self.stream):
            keys = self.engine.search_subset_batch_device(dq, handle, k, thrs, remap=True)
        self._keep = (dq, handle, keys)  # alive until the next call (the kernels run asynchronously)
        return keys

    # -- top-k distinct messages: this rank's slice of the global row -> message map, and its own best k messages -------------------------
    def set_row_messages(self, local_map: np.ndarray, n_messages: int) -> None:
        """This rank's slice of the row -> message map (message ordinals are global: no remap) with the GLOBAL n_messages."""
        with self.torch.cuda.stream(self.stream):
            self.engine.set_row_messages(local_map, n_messages)
        self.n_messages = int(n_messages)

    def _empty_rows(self):
        buf = getattr(self, "_no_rows", None)
        if buf is None:
            with self.torch.cuda.stream(self.stream):
                buf = self._no_rows = self.torch.empty(0, dtype=self.torch.int32, device=self._dev)
        return buf

    def _pinned_keys(self, shape):
        """the pinned host buffer of merged keys for `shape`, reused from call to call"""
        shape = tuple(int(n) for n in shape)
        pinned = self._pinned.get(shape)
        if pinned is None:
            pinned = self._pinned[shape] = self.torch.empty(shape, dtype=self.torch.int64).pin_memory()
        return pinned

    def local_top_messages(self, queries: np.ndarray, k: int, thrs, handle=None, masked: bool = False):
        """A batch of queries (host float32 [nq, dim]; thrs: one threshold per query) over this rank's shard, or, with `masked`, over a
        handle of `mask_to_device` (None: this rank's part of the mask is empty -> zero keys): ONE tavb_search_top_messages_device on
        the backend's stream -> keys [nq, k] carrying GLOBAL message ordinals.  Asynchronous."""
        if (masked and handle is None) or self.engine.rows == 0:
            return self._zero_keys(int(np.shape(queries)[0]), k)
        dq = self.stage_queries(np.ascontiguousarray(queries, dtype=np.float32))
        with self.torch.cuda.stream(self.stream):
            keys = self.engine.search_top_messages_device(dq, k, thrs, dev_rows=handle if masked else None)
        self._keep = (dq, handle, keys)  # alive until the next call (the kernels run asynchronously)
        return keys

    def merge_top_messages(self, gathered):
        """tensor int64 [world, nq, k] of top-messages lists -> [nq, k]: one maximum per message, then the best k (tavb_merge_top_messages_device)"""
        if not getattr(self, "n_messages", 0):
            raise RuntimeError("set_row_messages() first")
        with self.torch.cuda.stream(self.stream):
            return self.engine.merge_top_messages_device(gathered, self.n_messages)

    def search_top_messages_allgather(self, queries: np.ndarray, k: int, thrs, handle=None, masked: bool = False):
        """This rank's best k messages -> ncclAllGather -> the top-messages merge inside libtavb (tavb_search_top_messages_allgather), merged
        keys written into a reused pinned host buffer: -> int64 [nq, k] (host view, valid until the next call)."""
        dq = self.stage_queries(np.ascontiguousarray(queries, dtype=np.float32))
        pinned = self._pinned_keys((dq.shape[0], k))
        rows = None if not masked else (self._empty_rows() if handle is None else handle)
        with self.torch.cuda.stream(self.stream):
            self.engine.search_top_messages_allgather(dq, k, thrs, out_keys=pinned, dev_rows=rows)
        self.engine.synchronize()
        return pinned.numpy()

    def join_failed_top_messages(self, nq: int, k: int, n_messages: int) -> None:
        """What a rank does whose preparation of `search_top_messages_allgather` raised: the same collectives with failure lists.  The
        library refuses the call, before anything collective, on a context that was never told the message count (an error every rank
        makes alike there); a rank whose upload of its slice of the map is what failed has none yet, so it sets an empty map with the
        global count first -- the next lookup uploads the slice again."""
        with self.torch.cuda.stream(self.stream):
            if getattr(self, "n_messages", 0) != int(n_messages):
                self.engine.set_row_messages(np.zeros(0, dtype=np.int32), int(n_messages))
                self.n_messages = int(n_messages)
            self.engine.allgather_merge_top_messages(self.failed_lists(nq, k))
        self.engine.synchronize()

    def local_survivors(self, query: np.ndarray, thr: float):
        """every row of this shard with score >= thr -> (global ordinals int64, scores float32), unsorted (one emit-all pass)."""
        return self.engine.search_all(np.ascontiguousarray(query, dtype=np.float32), np.float32(thr), None)

    def keys_to_device(self, keys: np.ndarray):
        torch = self.torch
        with torch.cuda.stream(self.stream):
            return torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).to(self._dev)

    def search_allgather(self, queries, k: int, thr: float):
        """scan -> ncclAllGather -> merge inside libtavb, merged keys written into a reused pinned host buffer: -> int64 [nq, k] (host view,
        valid until the next call)."""
        pinned = self._pinned_keys((queries.shape[0], k))
        call = self.engine.search_allgather if _fused_k(k) else self.engine.search_topk_allgather
        call(queries, k, thr, out_keys=pinned)
        self.engine.synchronize()
        return pinned.numpy()

    def local_search(self, queries, k: int, thr: float):
        with self.torch.cuda.stream(self.stream):
            return (self.engine.search_device if _fused_k(k) else self.engine.search_topk_device)(queries, k, thr)

    def merge(self, gathered):
        with self.torch.cuda.stream(self.stream):
            return (self.engine.merge_device if _fused_k(gathered.shape[2]) else self.engine.merge_topk_device)(gathered)

    def to_host(self, keys) -> np.ndarray:
        # pinned staging buffer, reused: one async copy + one stream sync, no allocation per lookup
        pinned = self._pinned_keys(keys.shape)
        with self.torch.cuda.stream(self.stream):
            pinned.copy_(keys, non_blocking=True)
        self.stream.synchronize()
        return pinned.numpy().copy()

    def failed_lists(self, nq: int, k: int):
        """[nq, k] lists of PEER_FAILED_KEY: what a rank whose local search failed sends into the exchange.  A buffer of their own (never the
        gather buffer: with one rank that IS the collective's output), filled on the backend's stream -- the stream the exchange and the merge
        run on, so the fill is ordered in front of them."""
        buf = self._failed.get((nq, k))
        with self.torch.cuda.stream(self.stream):
            if buf is None:
                buf = self._failed[(nq, k)] = self.torch.empty((nq, k), dtype=self.torch.int64, device=self._dev)
            buf.fill_(PEER_FAILED_KEY)
        return buf

    def empty_gather(self, world: int, nq: int, k: int):
        shape = (world, nq, k)
        buf = self._gather.get(shape)
        if buf is None:
            with self.torch.cuda.stream(self.stream):
                buf = self.torch.empty(shape, dtype=self.torch.int64, device=self._dev)
            self._gather[shape] = buf
        return buf


@dataclass
class ShardedResult:
    ordinals: np.ndarray  # int64 [nq, k] global row ordinals
    scores: np.ndarray  # float32 [nq, k]
    counts: np.ndarray  # int32 [nq]


class ShardedSearcher:
    """Collective top-k over a row-sharded corpus.  Every rank calls `search` with the
    same queries (they are tiny next to the corpus: <= 3 MiB for 1024 x 1536 fp16, so the
    caller broadcasts/duplicates them) and every rank gets the same global result."""

    def __init__(self, backend: ShardBackend, group=None, always_collective: bool = False, gather_fn=None):
        import torch.distributed as dist

        self.dist = dist
        self.backend = backend
        self.group = group
        self.always_collective = always_collective  # run the all-gather even for one rank (tests)
        self.gather_fn = gather_fn  # test hook: (local [nq,k]) -> gathered [world,nq,k] by other means than RCCL
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0

    @property
    def native(self) -> bool:
        """the library's own communicator carries this searcher's exchanges (`gather_fn` overrides it)"""
        return bool(getattr(self.backend, "native_comm", False)) and self.gather_fn is None

    @property
    def collective(self) -> bool:
        """Does a call exchange?  With a communicator of the library, with `gather_fn`, with more than one rank, or when asked to
        (`always_collective` under an initialised torch.distributed).  Where it does not, `exchange` returns the local lists and an error
        of the local part is raised at once: nobody waits for this rank."""
        return self.native or self.gather_fn is not None or self.world > 1 or (self.always_collective and self.dist.is_initialized())

    def _merge_top_messages(self, gathered):
        """[world, nq, k] top-messages lists -> [nq, k] on the backend's device: the backend's own merge, or the host merge of libtavb"""
        if hasattr(self.backend, "merge_top_messages"):
            return self.backend.merge_top_messages(gathered)
        host = np.ascontiguousarray(self.backend.to_host(gathered)).view(np.uint64)
        return self.backend.keys_to_device(_native.merge_top_messages_keys(host))

    def exchange(self, local_keys, messages: bool = False):
        """this rank's sorted lists [nq, k] (global ordinals / positions) -> the lists merged over all ranks, on every rank.  messages: the
        keys carry MESSAGE ordinals -- one message may stand in several ranks' lists: one maximum per message, then the best k."""
        backend = self.backend
        nq, k = local_keys.shape
        # what differs by key family, chosen once: the library's call and the merge
        native_call = "allgather_merge_top_messages" if messages else ("allgather_merge" if _fused_k(k) else "allgather_merge_topk")
        merge = self._merge_top_messages if messages else backend.merge
        if self.native:
            return getattr(backend.engine, native_call)(local_keys)
        if self.gather_fn is not None:
            return merge(self.gather_fn(local_keys))
        if not self.collective:
            return local_keys
        gathered = backend.empty_gather(self.world, nq, k)
        # on the backend's stream, where it has one: behind the kernels that wrote `local_keys`, in front of the merge and `to_host`
        stream = getattr(backend, "stream", None)
        with contextlib.nullcontext() if stream is None else backend.torch.cuda.stream(stream):
            self.dist.all_gather_into_tensor(gathered.view(-1), local_keys.contiguous().view(-1), group=self.group)
        return merge(gathered)

    def _join(self, local, nq: int, k: int, messages: bool = False):
        """`local()` -> this rank's [nq, k] keys -> the exchange -> merged keys on the backend's device.  The protocol of tavb_search_allgather
        (include/tavb.h): a rank whose local part raises in a collective call joins the exchange with TAVB_KEY_PEER_FAILED in every slot
        and raises ITS error afterwards -- the peers are not left waiting in the all-gather."""
        failure = None
        try:
            keys = local()
        except Exception as exc:  # noqa: BLE001 -- whatever the backend or the caller's predicate raised
            if not self.collective:
                raise
            failure = exc
            keys = self.backend.failed_lists(nq, k)
        merged = self.exchange(keys, messages=True) if messages else self.exchange(keys)  # (`exchange` may be replaced by a one-argument hook)
        if failure is not None:
            raise failure
        return merged

    def lookup_keys(self, local, nq: int, k: int, messages: bool = False) -> np.ndarray:
        """The whole failure protocol, for every lookup form: `_join`, then the merged keys on the host (int64 [nq, k], a copy) -- or
        `PeerFailedError` where another rank joined with failure lists: nobody returns an answer that misses a shard."""
        return _raise_if_peer_failed(self.backend.to_host(self._join(local, nq, k, messages)))

    def search_keys(self, queries, k: int, min_score: float = 0.0):
        """-> backend tensor int64 [nq, k] of merged keys (still on the device, async)."""
        _check_k(k, "k")
        thr = float(_native.f32_threshold(min_score))
        return self._join(lambda: self.backend.local_search(queries, k, thr), int(queries.shape[0]), k)

    def search(self, queries, k: int, min_score: float = 0.0) -> ShardedResult:
        _check_k(k, "k")
        thr = float(_native.f32_threshold(min_score))
        if self.native:
            # the product path: one C-ABI call (no torch.distributed, no torch op), results land in pinned host memory
            keys = _raise_if_peer_failed(self.backend.search_allgather(queries, k, thr))
        else:
            keys = self.lookup_keys(lambda: self.backend.local_search(queries, k, thr), int(queries.shape[0]), k)
        return ShardedResult(*_native.decode_keys(keys))


class ShardedVectorBase:
    """VectorBase-shaped front end over a row-sharded corpus: every rank holds rows
    [row_offset, row_offset + local_rows) and every lookup is a collective call (all ranks pass the same
    query, all ranks get the same global answer).  Covers the lookup methods of the reference class
    (vectorbase.py:163-230: plain, batched, predicate and subset forms) and its storage methods (`add_embedding(s)`: appends go to the
    last rank's shard; `serialize` / `deserialize`: per-rank matrices; `clear`) -- all collective: every rank makes the same call."""

    def __init__(self, backend: ShardBackend, row_offset: int, local_rows: int, total_rows: int, group=None):
        self.backend = backend
        self.row_offset = int(row_offset)
        self.local_rows = int(local_rows)
        self.total_rows = int(total_rows)
        self.searcher = ShardedSearcher(backend, group=group)
        self._storage_dtype = backend.storage_dtype() if hasattr(backend, "storage_dtype") else "fp32"
        self._subset_cache = None  # (caller's subset object, private copy, total rows, ordinals int64, the backend's handle) of the last subset lookup
        self._row_messages = None  # the GLOBAL chunk row -> message map (set_row_messages), identical on every rank
        self._row_messages_layout = None  # the (total, offset, local) this rank's slice of it was last uploaded under

    def __len__(self) -> int:
        return self.total_rows

    def __bool__(self) -> bool:
        return True

    # ---- storage (collective: every rank makes the same call with the same arguments) ------------------------------------------------
    @property
    def _world(self) -> int:
        return self.searcher.world

    @property
    def _rank(self) -> int:
        return self.searcher.rank

    @property
    def _layout(self) -> tuple[int, int, int]:
        """(total rows, this rank's offset, this rank's rows): what device-resident handles -- subset, mask, message map -- were cut under"""
        return (self.total_rows, self.row_offset, self.local_rows)

    def add_embeddings(self, keys, embeddings) -> None:
        """vectorbase.py:130-148 over row shards: the new rows get the next global ordinals and go to the LAST rank's shard (contiguous
        ranges stay contiguous; only that rank uploads anything, and only the new rows); every rank advances its row count.  `keys` is
        accepted for signature compatibility (the reference caches key -> embedding in its model; there is no model here)."""
        rows = np.asarray(embeddings, dtype=np.float32)
        if rows.ndim != 2:
            raise ValueError(f"Expected 2D embeddings array, got {rows.ndim}D")
        if keys is not None and len(keys) != len(rows):
            raise ValueError(f"Number of keys {len(keys)} does not match number of embeddings {len(rows)}")
        if len(rows) == 0:
            return
        if self._rank == self._world - 1:
            self.backend.append_rows(rows)
            self.local_rows += len(rows)
        self.total_rows += len(rows)
        self._subset_cache = None
        # Appends always land on the last rank: contiguous ranges stay contiguous and nothing already placed moves -- but every collective
        # lookup waits for the largest shard, so an index GROWN by appends drifts towards single-GPU speed.  `imbalance()` says how far it has
        # drifted; `rebalance()` re-deals the rows (a collective: every rank hands its rows to `deserialize` of the balanced layout).

    def imbalance(self) -> float:
        """Collective: largest shard / mean shard (1.0 = balanced)."""
        if self.total_rows == 0 or self._world == 1:
            return 1.0
        counts = [None] * self._world
        self.searcher.dist.all_gather_object(counts, self.local_rows, group=self.searcher.group)
        return max(counts) / (self.total_rows / self._world)

    def rebalance(self, dtype: str | None = None) -> None:
        """Collective: re-deal the rows into balanced contiguous shards (`shard_range`), stored as they are now (`dtype` None: the dtype handed
        to `deserialize` / of the adopted shard tensor -- an fp16 index stays fp16: twice the HBM and other kernels otherwise).  Every rank serialises its rows, the ranks exchange
        them over torch.distributed (host side, every rank sees the whole matrix for a moment: a maintenance step for corpora that fit host memory,
        not the lookup path -- bigger ones are re-sharded from their source with `deserialize`) and each keeps its new range."""
        mine = self.serialize()
        if dtype is None:
            dtype = self._storage_dtype
        if self._world == 1:
            return
        parts = [None] * self._world
        self.searcher.dist.all_gather_object(parts, (self.row_offset, mine), group=self.searcher.group)
        parts = [p for p in parts if p[1].size]
        dim = parts[0][1].shape[1] if parts else 0
        whole = np.concatenate([p[1] for p in sorted(parts, key=lambda t: t[0])]) if parts else np.zeros((0, dim), np.float32)
        lo, hi = shard_range(len(whole), self._world, self._rank)
        self.deserialize(whole[lo:hi], dtype)

    def add_embedding(self, key, embedding) -> None:
        """vectorbase.py:115-128."""
        row = np.asarray(embedding, dtype=np.float32)
        if row.ndim == 1:
            row = row[None, :]
        if row.ndim != 2 or row.shape[0] != 1:
            raise ValueError(f"Expected a single embedding, got shape {row.shape}")
        self.add_embeddings(None if key is None else [key], row)

    def serialize(self) -> np.ndarray:
        """vectorbase.py:268-271, per rank: THIS rank's rows [row_offset, row_offset + local_rows) as a float32 matrix (a copy: the rows
        live on the device); `row_offset`, `local_rows`, `total_rows` place it in the whole.  Concatenating the ranks' matrices in rank
        order is the reference's `serialize()` of the whole index."""
        return self.backend.rows_to_host()

    def deserialize(self, local_data, dtype: str = "fp32") -> None:
        """vectorbase.py:273-287, per rank: every rank hands in ITS rows (float32 [n_r, dim], None or empty for none); the ranks agree on
        the offsets (an all-gather of the row counts over torch.distributed) and each uploads its own shard."""
        rows = np.zeros((0, 0), dtype=np.float32) if local_data is None else np.asarray(local_data, dtype=np.float32)
        if rows.ndim != 2:
            raise ValueError(f"Expected 2D embeddings array, got {rows.ndim}D")
        counts = [len(rows)]
        if self._world > 1:
            counts = [None] * self._world
            self.searcher.dist.all_gather_object(counts, len(rows), group=self.searcher.group)
        self.row_offset = int(sum(counts[: self._rank]))
        self.local_rows = len(rows)
        self.total_rows = int(sum(counts))
        self._storage_dtype = "fp16" if dtype == "fp16" else "fp32"
        self._subset_cache = None
        self.backend.set_rows(rows, self.row_offset, dtype)  # (no rows: the backend drops its shard)

    def clear(self) -> None:
        """vectorbase.py:248-255."""
        self.deserialize(None)

    @classmethod
    def from_device_shard(cls, device: int, shard_tensor, row_offset: int, total_rows: int, group=None):
        import torch.distributed as dist

        backend = DeviceShardBackend(device)
        backend.set_shard(shard_tensor, row_offset=row_offset)
        if dist.is_initialized() and group is None:
            backend.init_comm(dist.get_rank(), dist.get_world_size())
        return cls(backend, row_offset, shard_tensor.shape[0], total_rows, group=group)

    def _queries(self, q):
        a = np.ascontiguousarray(q, dtype=np.float32)
        if hasattr(self.backend, "stage_queries"):
            return self.backend.stage_queries(a)
        torch = getattr(self.backend, "torch", None)
        if torch is None:
            import torch as _t

            return _t.from_numpy(a)
        return torch.from_numpy(a).to(torch.device("cuda", self.backend.device))

    @staticmethod
    def _per_query(embeddings, thresholds=None):
        """-> (q float32 [nq, dim], the caller's threshold of every query: `thresholds` is one for all, or one per query)"""
        q = np.asarray(embeddings, dtype=np.float32)
        if q.ndim != 2:
            raise ValueError(f"Expected 2D embeddings array, got {q.ndim}D")
        per_query = thresholds is not None and not np.isscalar(thresholds) and np.ndim(thresholds) == 1
        if per_query and len(thresholds) != len(q):
            raise ValueError(f"Number of thresholds {len(thresholds)} does not match number of embeddings {len(q)}")
        return q, list(thresholds) if per_query else [thresholds] * len(q)

    def _batch_args(self, embeddings, max_k, thresholds, what: str):
        """The arguments of a batched lookup -> (q float32 [nq, dim], nq, k, float32 thresholds [nq]).  `max_k`: None -> 10, checked by
        `_check_k` under the parameter's name `what`; `thresholds`: one (None -> 0.0) or one per query.  Argument errors are the same on
        every rank and raise before anything collective."""
        q, each = self._per_query(embeddings, thresholds)
        k = 10 if max_k is None else int(max_k)
        _check_k(k, what)
        return q, len(q), k, np.asarray([_native.f32_threshold(0.0 if m is None else m) for m in each], dtype=np.float32)

    def fuzzy_lookup_embeddings(self, embeddings, max_hits: int | None = None, min_score: float | None = None):
        if max_hits is None:
            max_hits = 10
        if min_score is None:
            min_score = 0.0
        q, _ = self._per_query(embeddings)
        if self.total_rows == 0 or len(q) == 0:
            return [[] for _ in range(len(q))]  # (before max_hits is checked: an empty index answers max_hits = 0 too)
        _check_k(int(max_hits), "max_hits")  # (before anything collective: every rank makes the same call)
        res = self.searcher.search(self._queries(q), int(max_hits), min_score)
        from .vectorbase import _scored_lists  # (the lists are built in C: csrc/tavb_pyhits.c)

        return _scored_lists(res.ordinals, res.scores, res.counts, int(max_hits))

    def fuzzy_lookup_embedding(self, embedding, max_hits: int | None = None, min_score: float | None = None, predicate=None):
        """vectorbase.py:163-201.  With a predicate (:191-201): every rank applies it to the survivors of ITS shard, in ascending
        ordinal order (so the predicate is called once per survivor across the job, not once per survivor per rank), keeps its best
        `max_hits`, and the per-rank lists are merged like any other -- every rank returns the whole-corpus answer."""
        if predicate is None:
            return self.fuzzy_lookup_embeddings(np.asarray(embedding, dtype=np.float32)[None, :], max_hits, min_score)[0]
        from .vectorbase import ScoredInt

        k = 10 if max_hits is None else int(max_hits)
        if not (1 <= k <= _native.MAX_FUSED_K):
            raise ValueError(f"max_hits must be in 1..{_native.MAX_FUSED_K} for a sharded lookup with a predicate")
        thr = _native.f32_threshold(0.0 if min_score is None else min_score)
        if self.total_rows == 0:
            return []
        q = np.ascontiguousarray(embedding, dtype=np.float32)

        def local_lists():
            ids, scs = (np.zeros(0, np.int64), np.zeros(0, np.float32)) if self.local_rows == 0 else self.backend.local_survivors(q, thr)
            order = np.lexsort((ids,))  # ascending ordinal: the order of np.flatnonzero (:193)
            keep = np.fromiter((bool(predicate(int(i))) for i in ids[order]), dtype=bool, count=len(order))
            local = np.zeros((1, k), dtype=np.uint64)
            best = np.sort(_pack_keys(scs[order][keep], ids[order][keep]))[::-1][:k]
            local[0, : len(best)] = best
            return self.backend.keys_to_device(local)

        ords, sc, cnt = _native.decode_keys(self.searcher.lookup_keys(local_lists, 1, k))
        return [ScoredInt(int(o), float(s_)) for o, s_ in zip(ords[0, : cnt[0]].tolist(), sc[0, : cnt[0]].tolist())]

    def fuzzy_lookup_embedding_in_subset(self, embedding, ordinals_of_subset, max_hits: int | None = None, min_score: float | None = None):
        """vectorbase.py:203-230 over the row-sharded corpus: every rank gathers the rows of the caller's subset that lie in its shard,
        the per-rank top-k lists (keys carrying POSITIONS in the caller's list: duplicates and negative, wrapping ordinals behave as in
        the reference) are merged over the ranks; returns the caller's ordinals."""
        from .vectorbase import ScoredInt

        k = 10 if max_hits is None else int(max_hits)
        _check_k(k, "max_hits")
        thr = float(_native.f32_threshold(0.0 if min_score is None else min_score))
        if len(ordinals_of_subset) == 0 or self.total_rows == 0:
            return []
        q = np.ascontiguousarray(embedding, dtype=np.float32)
        # the same subset object with the same content again (the memory provider's scope list per query term,
        # storage/memory/messageindex.py:173-183): this shard's part of it stays on the device (as VectorBase does it)
        layout = self._layout
        cached = self._subset_cache
        resident = hasattr(self.backend, "subset_to_device") and isinstance(ordinals_of_subset, (list, np.ndarray))
        if (resident and cached is not None and cached[0] is ordinals_of_subset and cached[2] == layout and len(cached[1]) == len(ordinals_of_subset)
                and (np.array_equal(cached[1], ordinals_of_subset) if isinstance(ordinals_of_subset, np.ndarray) else cached[1] == ordinals_of_subset)):
            subset = cached[3]
            handle = cached[4]

            def local_lists():
                return self.backend.local_search_subset_resident(q, handle, k, thr)
        else:
            subset = np.asarray(ordinals_of_subset)
            if subset.dtype.kind not in "iu":
                raise IndexError("arrays used as indices must be of integer (or boolean) type")
            subset = subset.astype(np.int64, copy=False).reshape(-1)
            n = self.total_rows
            rows = np.where(subset < 0, subset + n, subset)  # numpy index wrap (:218)
            bad = (rows < 0) | (rows >= n)
            if bad.any():
                raise IndexError(f"index {int(subset[np.argmax(bad)])} is out of bounds for axis 0 with size {n}")
            mine = np.flatnonzero((rows >= self.row_offset) & (rows < self.row_offset + self.local_rows))  # ascending positions: lists stay sorted among ties
            # (argument errors above are the same on every rank -- every rank holds the same list -- and raise before anything collective)
            if resident:
                def local_lists():
                    handle = self.backend.subset_to_device(rows[mine] - self.row_offset, mine)
                    is_array = isinstance(ordinals_of_subset, np.ndarray)
                    keep = subset.copy() if is_array else subset
                    self._subset_cache = (ordinals_of_subset, ordinals_of_subset.copy() if is_array else list(ordinals_of_subset), layout, keep, handle)
                    return self.backend.local_search_subset_resident(q, handle, k, thr)
            else:
                def local_lists():
                    return self.backend.local_search_subset(q, rows[mine] - self.row_offset, mine, k, thr)
        pos, sc, cnt = _native.decode_keys(self.searcher.lookup_keys(local_lists, 1, k))
        return [ScoredInt(int(subset[p]), float(s_)) for p, s_ in zip(pos[0, : cnt[0]].tolist(), sc[0, : cnt[0]].tolist())]

    # ---- masked lookups: with a backend that offers `mask_to_device` / `local_search_masked`, this rank's slice of the mask stays on its
    # device and a batch is ONE exchange; any other backend: the subset lookup per query over np.flatnonzero(mask), collective like it
    def _masked_backend(self):
        backend = getattr(self, "backend", None)
        return backend if hasattr(backend, "mask_to_device") and hasattr(backend, "local_search_masked") else None

    def row_mask(self, allowed):
        """An allow-mask (bool array / sequence / torch bool tensor of length len(self), the same on every rank) -> a `RowMask` tied to
        this index at this length.  With a backend that expands masks itself it holds this rank's allowed rows on the device, the GLOBAL
        count, the layout they were cut under and the whole mask packed to bits on the host (rows / 8 bytes; a tensor on the backend's
        device is packed there and only its bits are copied out); otherwise np.flatnonzero of the mask.  No collective."""
        from .vectorbase import RowMask

        backend = self._masked_backend()

        def device_mask(mask, bits, count):
            """the device-backed form: this rank's slice of `mask` expanded on its device, the whole mask as `bits`, the GLOBAL count"""
            local = mask[self.row_offset : self.row_offset + self.local_rows]
            return RowMask(self, self.total_rows, count, dev_rows=backend.mask_to_device(local), layout=self._layout, bits=bits)

        if hasattr(allowed, "is_cuda") and hasattr(allowed, "dtype"):  # a torch tensor
            if "bool" not in str(allowed.dtype):
                raise TypeError(f"a mask must be bool, got {allowed.dtype}")
            on_device = (backend is not None and allowed.is_cuda and hasattr(backend, "engine") and (allowed.device.index or 0) == getattr(backend, "device", None)
                         and allowed.dim() == 1 and allowed.shape[0] == self.total_rows and self.total_rows > 0)
            if on_device:
                # the mask was made on the caller's stream: wait for it BEFORE entering the backend's stream (the engine's own), where
                # Engine.pack_mask_tensor's synchronise of the "current" stream no longer means the caller's.  Every rank must pack the
                # finished mask: the global count decides whether a rank joins the exchange.
                backend.torch.cuda.current_stream(backend.device).synchronize()
                with backend.torch.cuda.stream(backend.stream):
                    bits = backend.engine.pack_mask_tensor(allowed).cpu().numpy().view(np.uint32)
                return device_mask(allowed, bits, _popcount(bits))
            allowed = allowed.cpu().numpy()
        a = np.asarray(allowed)
        if a.dtype != np.bool_:
            raise TypeError(f"a mask must be bool, got {a.dtype}")
        if a.ndim != 1 or a.shape[0] != self.total_rows:
            raise ValueError(f"mask covers {a.shape[0] if a.ndim else 0} rows, the index has {self.total_rows}")
        if backend is not None:
            return device_mask(a, _native.pack_mask_bits(a), int(np.count_nonzero(a)))
        flat = np.flatnonzero(a)
        return RowMask(self, self.total_rows, len(flat), flat=flat)

    def _resolve_mask(self, allowed):
        from .vectorbase import RowMask

        if not isinstance(allowed, RowMask):
            return self.row_mask(allowed)
        if allowed._owner() is not self:
            raise ValueError("this RowMask was built by another index")
        if allowed.rows != self.total_rows:
            raise ValueError(f"mask covers {allowed.rows} rows, the index has {self.total_rows}")
        return allowed

    def _mask_part(self, mask, backend):
        """This rank's part of a device-backed mask as the backend's handle (None: an empty part).  A handle cut under another layout
        (the rows were re-dealt since) is cut again from its packed bits: this rank's slice, expanded on its device.  May raise on ONE
        rank: call it inside the local part of a collective."""
        layout = self._layout
        if mask.layout != layout:
            lo, n = self.row_offset, self.local_rows
            part = np.unpackbits(mask.bits.view(np.uint8)[lo // 8 : (lo + n + 7) // 8], bitorder="little")[lo % 8 : lo % 8 + n]
            mask.dev_rows = backend.mask_to_device(part.astype(np.bool_))
            mask.layout = layout
        return mask.dev_rows

    def fuzzy_lookup_embeddings_masked(self, embeddings, allowed, max_hits: int | None = None, min_score=None):
        """≡ [fuzzy_lookup_embedding_in_subset(e, np.flatnonzero(allowed), max_hits, min_score) for e in embeddings] (`min_score`: one
        threshold, or one per query); `allowed`: a mask or the `RowMask` made from one.  With a backend that offers the masked route the
        whole batch is one local call per rank and ONE exchange (a rank whose part of the mask is empty still joins); a handle cut under
        another layout (`rebalance()`) is cut again from its packed bits, on every rank alike and without a collective."""
        from .vectorbase import _scored_lists

        backend = self._masked_backend()
        if backend is not None:
            q, nq, k, thr = self._batch_args(embeddings, max_hits, min_score, "max_hits")
            mask = self._resolve_mask(allowed)
            if mask.bits is not None:
                if mask.count == 0 or nq == 0 or self.total_rows == 0:
                    return [[] for _ in range(nq)]  # (the global count is the same on every rank: nobody waits in an exchange)

                def local_lists():
                    return backend.local_search_masked(q, self._mask_part(mask, backend), k, thr)

                return _scored_lists(*_native.decode_keys(self.searcher.lookup_keys(local_lists, nq, k)), k)
        # no masked route: the subset lookup per query, which checks max_hits and converts the threshold itself
        q, each = self._per_query(embeddings, min_score)
        flat = self._resolve_mask(allowed).flat()
        return [self.fuzzy_lookup_embedding_in_subset(e, flat, max_hits, each[i]) for i, e in enumerate(q)]

    def fuzzy_lookup_embedding_masked(self, embedding, allowed, max_hits: int | None = None, min_score: float | None = None):
        e = np.asarray(embedding, dtype=np.float32)
        if e.ndim != 1:
            raise ValueError(f"Expected 1D embedding, got {e.ndim}D")
        return self.fuzzy_lookup_embeddings_masked(e[None, :], allowed, max_hits, min_score)[0]

    # ---- top-k distinct messages ------------------------------------------------------------------------------------------------------
    def set_row_messages(self, row_to_message) -> None:
        """The GLOBAL chunk row -> message ordinal map (-1: none), identical on every rank; n_messages = its largest ordinal + 1 over the
        index' rows.  With a backend that has an engine this rank's slice is uploaded before the next top-messages lookup, and again
        whenever the layout changes (`rebalance`, appends).  No collective."""
        self._row_messages = np.array(row_to_message, dtype=np.int64).reshape(-1)  # a snapshot: never an alias of the caller's array
        self._row_messages_layout = None

    def _n_messages(self) -> int:
        held = self._row_messages[: self.total_rows]
        return max(int(held.max()) + 1, 0) if len(held) else 0

    def _sync_row_messages(self) -> None:
        """this rank's slice of the map on its device, under the current layout (may raise on ONE rank: call it inside the local part)"""
        layout = self._layout
        if self._row_messages_layout != layout and hasattr(self.backend, "set_row_messages"):
            self.backend.set_row_messages(self._row_messages[self.row_offset : self.row_offset + self.local_rows], self._n_messages())
        self._row_messages_layout = layout

    @staticmethod
    def _message_keys(msgs: np.ndarray, scs: np.ndarray, k: int) -> np.ndarray:
        """(message ordinal, float32 score) pairs -> the sorted, zero-padded top-messages list uint64 [k]: per message its best score"""
        keep = msgs >= 0
        keys = np.sort(_pack_keys(scs[keep], msgs[keep]))[::-1]
        _, first = np.unique(keys & np.uint64(0xFFFFFFFF), return_index=True)  # a message's first key in that order is its largest
        best = keys[np.sort(first)][:k]
        out = np.zeros(k, dtype=np.uint64)
        out[: len(best)] = best
        return out

    def lookup_top_messages_by_embeddings(self, embeddings, max_messages: int | None = None, threshold_score=None, allowed=None):
        """`VectorBase.lookup_top_messages_by_embeddings` over the row-sharded corpus (collective: every rank passes the same arguments and
        gets the same lists): per query the `max_messages` (None -> 10; 1 .. 16384) messages with the highest best score among the rows
        that pass `threshold_score` (one, or one per query) and lie inside `allowed` (a mask or a `RowMask` of this index; None: every
        row), sorted by (score descending, message ordinal ascending).  Needs `set_row_messages`.  Every rank returns ITS best
        `max_messages` messages -- a message of the whole-corpus answer is among those of the rank that holds its best row, with that
        score -- and ONE exchange per batch merges them: one maximum per message, then the best `max_messages`.  With the library's own
        communicator that is one C call (tavb_search_top_messages_allgather); with `gather_fn` or torch.distributed the backend's
        `local_top_messages` / `merge_top_messages` around the exchange; a backend without them: `local_survivors` and a collapse on the
        host.  A rank whose local part raises joins the exchange with failure lists and raises its own error; the others raise
        `PeerFailedError`."""
        from .vectorbase import _scored_lists

        q, nq, k, thr = self._batch_args(embeddings, max_messages, threshold_score, "max_messages")
        if self._row_messages is None:
            raise RuntimeError("set_row_messages() first")
        if len(self._row_messages) < self.total_rows:
            raise ValueError(f"the row -> message map covers {len(self._row_messages)} rows, the index has {self.total_rows}")
        mask = None if allowed is None else self._resolve_mask(allowed)
        # (global quantities only: every rank decides alike, nobody waits in an exchange)
        if nq == 0 or self.total_rows == 0 or self._n_messages() == 0 or (mask is not None and mask.count == 0):
            return [[] for _ in range(nq)]
        backend = self.backend
        on_device = hasattr(backend, "local_top_messages") and (mask is None or mask.bits is not None)

        def handle():
            return None if mask is None else self._mask_part(mask, backend)

        if on_device and self.searcher.native and hasattr(backend, "search_top_messages_allgather"):
            try:  # the product path: one C call; what can fail on ONE rank before it still joins the collectives -- `join_failed_top_messages`
                # is those collectives with failure lists, not a copy of `ShardedSearcher.lookup_keys`
                self._sync_row_messages()
                rows = handle()
            except Exception:  # noqa: BLE001
                self._row_messages_layout = None
                backend.join_failed_top_messages(nq, k, self._n_messages())
                raise
            keys = _raise_if_peer_failed(backend.search_top_messages_allgather(q, k, thr, rows, masked=mask is not None))
            return _scored_lists(*_native.decode_keys(keys), k)

        if on_device:
            def local_lists():
                self._sync_row_messages()
                return backend.local_top_messages(q, k, thr, handle(), masked=mask is not None)
        else:
            flat = None if mask is None else mask.flat()

            def local_lists():
                lo, hi = self.row_offset, self.row_offset + self.local_rows
                allowed_rows = None if flat is None else flat[(flat >= lo) & (flat < hi)]
                local = np.zeros((nq, k), dtype=np.uint64)
                for i in range(nq):
                    if self.local_rows == 0 or (allowed_rows is not None and len(allowed_rows) == 0):
                        continue
                    ids, scs = backend.local_survivors(q[i], thr[i])
                    ids, scs = np.asarray(ids, dtype=np.int64), np.asarray(scs, dtype=np.float32)
                    if allowed_rows is not None:
                        keep = np.isin(ids, allowed_rows)
                        ids, scs = ids[keep], scs[keep]
                    local[i] = self._message_keys(self._row_messages[ids], scs, k)
                return backend.keys_to_device(local)

        return _scored_lists(*_native.decode_keys(self.searcher.lookup_keys(local_lists, nq, k, messages=True)), k)

    def lookup_top_messages_by_embedding(self, embedding, max_messages: int | None = None, threshold_score: float | None = None, allowed=None):
        """The one-query form of `lookup_top_messages_by_embeddings`."""
        e = np.asarray(embedding, dtype=np.float32)
        if e.ndim != 1:
            raise ValueError(f"Expected 1D embedding, got {e.ndim}D")
        return self.lookup_top_messages_by_embeddings(e[None, :], max_messages, threshold_score, allowed)[0]

    def lookup_messages_by_embedding(self, embedding, row_to_message, max_matches: int | None = None, threshold_score: float | None = None, accept=None):
        """`SqliteMessageTextIndex.lookup_by_embedding` / `lookup_in_subset_by_embedding` (storage/sqlite/messageindex.py:296-326, 182-257)
        over the sharded corpus: the whole-corpus top-`max_matches` chunk rows (collective), THEN the provider's message filter and
        best-score-per-message aggregation on the merged hits (`row_to_message`: the GLOBAL chunk row -> message map; identical on
        every rank, so every rank returns the same messages)."""
        from .adapters import best_score_per_message

        hits = self.fuzzy_lookup_embedding(embedding, max_hits=max_matches, min_score=threshold_score)
        members = None if accept is None else (accept if callable(accept) else set(int(x) for x in accept).__contains__)
        return best_score_per_message(hits, row_to_message, max_matches, members)
