"""Drop-in for `typeagent.aitools.vectorbase` with the nearest-neighbour search
running on MI355X (gfx950) through libtavb.so.

API mirror of the reference's `src/typeagent/aitools/vectorbase.py`
(/root/reference; line numbers below refer to it):

  DEFAULT_MIN_SCORE, MODEL_DEFAULT_MIN_SCORES, get_default_min_score   :16-41
  cosine_to_score                                                      :44-47
  ScoredInt                                                            :50-55
  TextEmbeddingIndexSettings                                           :58-79
  VectorBase                                                           :82-287

Same names, arguments, defaults, return types and exceptions.  What differs is
where the arithmetic runs: `fuzzy_lookup_embedding*` launch HIP kernels (fused
dot + score + threshold + top-k) instead of np.dot/argpartition, and there are
additive methods: `fuzzy_lookup_embeddings` (a batch of queries in one
submission), the masked lookups (`row_mask`, `fuzzy_lookup_embedding_masked`,
`fuzzy_lookup_embeddings_masked`: search only among the rows an allow-mask names) and the scoped message lookups (`message_mask`,
`lookup_messages_by_embedding(s)_masked`, `lookup_messages_by_embeddings`: a scope of message ordinals searched as a mask, batches aggregated to messages).  The host ndarray `_vectors` stays the authoritative copy for
serialize()/deserialize(); the device buffer mirrors it and is synced lazily,
appends moving only the new rows.

There is no CPU fallback: a lookup on a non-empty index without libtavb.so or
without a visible MI355X raises RuntimeError.

Documented deviations from the reference (none is exercised by its callers):
  * equal float32 scores are ordered by ascending ordinal (the reference's order
    among ties is whatever numpy's introselect leaves, :183-187);
  * a query is converted to float32 (np.dot would promote a float64 query);
  * negative `max_hits` raises ValueError (the reference returns slicing artefacts).
"""

from __future__ import annotations

import ctypes
import gc
import os
import time
import weakref
from collections.abc import Callable
from dataclasses import dataclass

import numpy as np

from . import _native
from .embeddings import IEmbeddingModel, NormalizedEmbedding, NormalizedEmbeddings

DEFAULT_MIN_SCORE = 0.85

# Per-model score cut-offs the reference ships for the built-in OpenAI models (:31-35).
MODEL_DEFAULT_MIN_SCORES: dict[str, float] = {
    "text-embedding-3-large": 0.74,
    "text-embedding-3-small": 0.73,
    "text-embedding-ada-002": 0.93,
}

_PAGE = _native.MAX_FUSED_K  # most hits the fused select-while-streaming kernels return; beyond: the exact large-k route up to MAX_LARGE_K (`_large_k`), then the sorted device route (`_sort_all`)


try:  # whole-matrix digests of the "full" host watch
    from xxhash import xxh3_128_digest as _digest
except Exception:  # pragma: no cover - xxhash is part of the image
    import hashlib

    def _digest(data) -> bytes:
        return hashlib.blake2b(data, digest_size=16).digest()


class _Watch:
    """Dirty flag shared by an index and every view of its host matrix it has handed out (and by the indexes that adopted such a
    view through deserialize(): `followers`)."""

    __slots__ = ("dirty", "followers")

    def __init__(self) -> None:
        self.dirty = False
        self.followers: list[_Watch] = []

    def touch(self) -> None:
        self.dirty = True
        for f in self.followers:
            f.dirty = True


class _WatchedMatrix(np.ndarray):
    """What serialize() / `_vectors` / get_embedding_at() hand out for a matrix this index owns: a plain float32 view of the live
    host matrix (the reference hands out the live `_vectors`, vectorbase.py:268-271) that remembers being written to.  The
    reference always scores the live matrix (:176); here the device mirror is refreshed on the next lookup after a write made
    through numpy's array API on this array or on a view derived from it: item / slice assignment, in-place operators and ufunc
    `out=`, fill / sort / put / ..., np.copyto / np.put / np.place / np.putmask, `out=` / `dst=` of any other numpy function, `.flat`
    (touching `.flat` counts as a write: the iterator it returns assigns behind numpy's back).
    Arrays that merely DERIVE from the matrix but own their memory (m.copy(), m * 2, a matrix product with it) are plain results: writing to them
    does not mark anything.  What this class cannot see -- a base-class view from np.asarray(), memoryview, ctypes pointers, torch.from_numpy,
    another library writing through the buffer protocol -- is caught by the fingerprint the index keeps of a matrix it has handed out
    (`verify_host`: sampled rows by default, so a bulk rewrite is noticed, a single-row edit by such a route is not): those writers
    call `VectorBase.mark_dirty()`."""

    _tavb_watch: _Watch | None = None

    def __array_finalize__(self, obj) -> None:
        # only arrays that SHARE the matrix' memory inherit the watch (a copy that owns its data is nobody's mirror: editing it must not
        # trigger a re-upload of a multi-GB corpus)
        if obj is not None and not self.flags.owndata:
            self._tavb_watch = getattr(obj, "_tavb_watch", None)

    def _touch(self) -> None:
        w = self._tavb_watch
        if w is not None:
            w.touch()

    def __setitem__(self, key, value) -> None:
        self._touch()
        super().__setitem__(key, value)

    @property
    def flat(self):
        self._touch()  # `m.flat[i] = x` assigns through a np.flatiter: conservative, also for reads
        return np.ndarray.flat.__get__(self)

    @flat.setter
    def flat(self, value) -> None:
        self._touch()
        np.ndarray.flat.__set__(self, value)

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        plain = lambda a: a.view(np.ndarray) if isinstance(a, _WatchedMatrix) else a
        if out is not None:
            for o in out:
                if isinstance(o, _WatchedMatrix):
                    o._touch()
            kwargs["out"] = tuple(plain(o) for o in out)
        if method == "at" and isinstance(inputs[0], _WatchedMatrix):
            inputs[0]._touch()
        result = getattr(ufunc, method)(*(plain(i) for i in inputs), **kwargs)
        if out is not None and method == "__call__" and len(out) == 1:
            return out[0]  # `m *= 2` must rebind m to itself
        return result  # plain ndarrays: results of arithmetic on the matrix are copies, not watched

    def __array_function__(self, func, types, args, kwargs):
        if func in _WRITING_FUNCTIONS and args and isinstance(args[0], _WatchedMatrix):
            args[0]._touch()
        for name in ("out", "dst", "a"):  # np.take(..., out=m), a product written into out=m, np.copyto(dst=m, src=...), np.put(a=m, ...)
            target = kwargs.get(name)
            if name == "a" and func not in _WRITING_FUNCTIONS:
                continue
            for t in target if isinstance(target, tuple) else (target,):
                if isinstance(t, _WatchedMatrix):
                    t._touch()
        result = super().__array_function__(func, types, args, kwargs)
        if isinstance(result, _WatchedMatrix) and result.flags.owndata:
            return result.view(np.ndarray)  # a fresh array (a product, a sorted copy, ...): nobody's mirror
        return result

    def _writing_method(name):  # noqa: N805 -- class-body helper
        base = getattr(np.ndarray, name)

        def method(self, *args, **kwargs):
            self._touch()
            return base(self, *args, **kwargs)

        method.__name__ = name
        return method

    fill = _writing_method("fill")
    sort = _writing_method("sort")
    partition = _writing_method("partition")
    put = _writing_method("put")
    setfield = _writing_method("setfield")
    byteswap = _writing_method("byteswap")
    del _writing_method


_WRITING_FUNCTIONS = {np.copyto, np.put, np.place, np.putmask, np.put_along_axis, np.fill_diagonal}


def get_default_min_score(model_name: str) -> float:
    return MODEL_DEFAULT_MIN_SCORES.get(model_name, DEFAULT_MIN_SCORE)


def cosine_to_score(cosine_similarity: np.ndarray) -> np.ndarray:
    """Host-side statement of the score map the kernels apply per row: cosine in
    [-1, 1] -> public score in [0, 1]."""
    return np.clip((cosine_similarity + 1.0) / 2.0, 0.0, 1.0)


@dataclass(slots=True)  # same fields / equality / repr as the reference's (vectorbase.py:50-55); slots halve the cost of building 32k hits per 1024-query batch
class ScoredInt:
    item: int
    score: float


def _default_embedding_model() -> IEmbeddingModel:
    # The reference builds its default provider model here (:74, model_adapters
    # .create_embedding_model).  That is LLM/HTTP plumbing outside this package: use the
    # reference's factory when typeagent is importable, otherwise insist on an explicit model.
    try:
        from typeagent.aitools.model_adapters import create_embedding_model  # type: ignore
    except Exception as exc:  # pragma: no cover - depends on the host environment
        raise RuntimeError(
            "TextEmbeddingIndexSettings needs an explicit embedding_model when typeagent's "
            "model_adapters is not importable"
        ) from exc
    return create_embedding_model()


@dataclass
class TextEmbeddingIndexSettings:
    embedding_model: IEmbeddingModel
    min_score: float  # 0..1
    max_matches: int | None  # >= 1, None = no limit
    batch_size: int  # >= 1

    def __init__(
        self,
        embedding_model: IEmbeddingModel | None = None,
        min_score: float | None = None,
        max_matches: int | None = None,
        batch_size: int | None = None,
    ):
        self.embedding_model = embedding_model or _default_embedding_model()
        name = getattr(self.embedding_model, "model_name", "")
        self.min_score = get_default_min_score(name) if min_score is None else min_score
        self.max_matches = max_matches if (max_matches and max_matches >= 1) else None
        self.batch_size = batch_size if (batch_size and batch_size >= 1) else 8


def _env_dtype() -> int:
    v = os.environ.get("TYPEAGENT_VB_DTYPE", "fp32").lower()
    if v in ("fp16", "f16", "half"):
        return _native.TAVB_F16
    return _native.TAVB_F32


try:  # the C builder of the hit lists (csrc/tavb_pyhits.c, built next to libtavb.so); host-side only -- the Python loop below does the same work
    from . import _tavb_pyhits
except ImportError:  # pragma: no cover - the module ships with the package
    _tavb_pyhits = None


def _scored_lists(ords: np.ndarray, scs: np.ndarray, cnts: np.ndarray, width: int) -> list[list[ScoredInt]]:
    """[Q, width] result arrays -> Q lists of ScoredInt (what vectorbase.py:188-190 builds per query).  A 1024 x 32 batch is 32k
    Python objects: the cyclic collector would wake ~45 times while they are allocated (none of them can be part of a cycle: an
    int and a float each) -- it is paused for the duration when it was on and the batch is big.  The objects are built in C
    (`_tavb_pyhits.build`: tp_alloc + two slot stores per hit, ~45 ns against ~110 ns through the dataclass __init__)."""
    pause = len(cnts) * width >= 4096 and gc.isenabled()
    if pause:
        gc.disable()
    try:
        if _tavb_pyhits is not None and ords.dtype == np.int64 and scs.dtype == np.float32 and cnts.dtype == np.int32 \
                and ords.flags.c_contiguous and scs.flags.c_contiguous and cnts.flags.c_contiguous and ords.shape == scs.shape == (len(cnts), width):
            return _tavb_pyhits.build(ScoredInt, ords, scs, cnts, width)
        rows_o, rows_s = ords.tolist(), scs.tolist()
        counts = cnts.tolist()
        return [list(map(ScoredInt, o, s_)) if m == width else list(map(ScoredInt, o[:m], s_[:m])) for o, s_, m in zip(rows_o, rows_s, counts)]
    finally:
        if pause:
            gc.enable()


def _sorted_lists(ords: np.ndarray, scs: np.ndarray, cnts: np.ndarray) -> list[list[ScoredInt]]:
    """The concatenated results of a sorted lookup (`Engine.search_sorted`: query q's counts[q] hits after those of the queries before
    it) -> one list of ScoredInt per query, each built by `_scored_lists` from a [1, m] view."""
    out, off = [], 0
    for m in cnts.tolist():
        out.append(_scored_lists(ords[None, off:off + m], scs[None, off:off + m], np.array([m], np.int32), m)[0] if m else [])
        off += m
    return out


class RowMask:
    """What `VectorBase.row_mask(allowed)` returns: the allowed rows of ONE index at ONE length, expanded once and kept where the lookups
    read them -- on a single-GPU engine an int32 row list in device memory (`dev_rows`, ascending; `count` of them), so that a masked
    lookup sends only its queries.  `rows` is the index length the mask was built for: a handle used after the index grew or shrank
    raises ValueError, and so does one used after `VectorBase.remove_rows` removed a row, whatever the length is by then (`epoch`).  `flat()` is np.flatnonzero of the mask, made on first use; only the fallback route needs it.  On a device group the
    handle holds one shard-local list per device (`shards`, cut by `bounds`), on a row-sharded index this rank's list and the packed mask.
    A single-GPU engine also keeps the packed mask on the device (`dev_bits`, int32 words: row r = bit r & 31 of word r >> 5) and
    `span` = (first, last) allowed row, read once when the handle is built (or handed in as `span=` by the scope algebra, whose kernels
    report it): what a batch on the 32/64-query tile reads instead of the list.  Handles of one index combine: `a & b`, `a | b`, `a - b`,
    `~a` (`VectorBase.intersect_masks` / `union_masks`)."""

    __slots__ = ("rows", "count", "dev_rows", "dev_bits", "span", "shards", "bounds", "layout", "bits", "epoch", "_flat", "_owner", "_plans")

    def __init__(self, owner, rows: int, count: int, dev_rows=None, flat: np.ndarray | None = None, shards=None, bounds=None, layout=None, bits=None,
                 dev_bits=None, span=None):
        self.rows = int(rows)
        self.count = int(count)
        # the owner's removal epoch (`VectorBase.remove_rows` bumps it): the same length after a removal and an append is not the same rows
        self.epoch = getattr(owner, "_removal_epoch", 0)
        self.dev_rows = dev_rows
        self.dev_bits = dev_bits
        if span is not None:  # the scope algebra's kernels report it with the count: nothing is read back
            self.span = (int(span[0]), int(span[1])) if self.count > 0 else None
        else:
            self.span = (int(dev_rows[0]), int(dev_rows[-1])) if dev_bits is not None and dev_rows is not None and self.count > 0 else None
        self._plans: dict = {}  # (queries, max_hits, the engine's mask_tile options) -> tile route or not: a handle is searched again and again
        # a device group (multidevice.DeviceGroup.mask_to_rows): one shard-local int32 row list per device (None: no allowed row there)
        # and the shard bounds the mask was cut by
        self.shards = shards
        self.bounds = None if bounds is None else tuple(bounds)
        # a row-sharded index (sharded.ShardedVectorBase): dev_rows = THIS rank's local rows, `count` the global count, `layout` =
        # (total_rows, row_offset, local_rows) they were cut under, `bits` the whole mask packed on the host (rows / 8 bytes, pack_mask_bits)
        self.layout = layout
        self.bits = bits
        self._flat = flat
        self._owner = weakref.ref(owner)

    def __len__(self) -> int:
        return self.count

    def flat(self) -> np.ndarray:
        if self._flat is None:
            if self.bits is not None:
                self._flat = np.flatnonzero(np.unpackbits(self.bits.view(np.uint8), bitorder="little")[: self.rows]).astype(np.int64)
            elif self.shards is not None:
                parts = [r.cpu().numpy().astype(np.int64) + lo for r, lo in zip(self.shards, self.bounds) if r is not None]
                self._flat = np.concatenate(parts) if parts else np.zeros(0, np.int64)
            else:
                self._flat = np.zeros(0, np.int64) if self.dev_rows is None else self.dev_rows.cpu().numpy().astype(np.int64)
        return self._flat

    # AND / OR / difference / complement with the masks of the same index at the same length (`VectorBase.intersect_masks` and the rest): on
    # a single-GPU engine the packed masks are combined on the device and the result is a full handle
    def _index(self):
        owner = self._owner()
        if owner is None:
            raise ValueError("the index this RowMask was built by is gone")
        return owner

    def __and__(self, other) -> "RowMask":
        return self._index().intersect_masks(self, other)

    def __or__(self, other) -> "RowMask":
        return self._index().union_masks(self, other)

    def __sub__(self, other) -> "RowMask":
        return self._index()._combine_masks(_native.MASK_ANDNOT, (self, other))

    def __invert__(self) -> "RowMask":
        return self._index()._combine_masks(_native.MASK_ANDNOT, (self,))


def _is_tensor(x) -> bool:
    return hasattr(x, "is_cuda") and hasattr(x, "dtype")  # a torch tensor, without importing torch for callers that never pass one


class VectorBase:
    settings: TextEmbeddingIndexSettings
    _model: IEmbeddingModel
    _embedding_size: int

    def __init__(
        self,
        settings: TextEmbeddingIndexSettings,
        *,
        device: int | None = None,
        corpus_dtype: str | None = None,
        devices: list[int] | None = None,
        keep_host_copy: bool | None = None,
        verify_host: str | None = None,
    ):
        self.settings = settings
        self._model = settings.embedding_model
        self._embedding_size = 0
        self._device_index = device if device is not None else (int(os.environ["TYPEAGENT_VB_DEVICE"]) if "TYPEAGENT_VB_DEVICE" in os.environ else None)
        # several GPUs under ONE object (row shards, one context + stream per device; typeagent_py_amd/multidevice.py)
        if devices is None and os.environ.get("TYPEAGENT_VB_DEVICES"):
            devices = [int(x) for x in os.environ["TYPEAGENT_VB_DEVICES"].split(",") if x.strip() != ""]
        self._devices = list(devices) if devices else None
        # keep_host_copy=False: rows handed to add_embedding(s) are streamed straight into the device corpus (pinned
        # staging, async H2D, on-device fp16 conversion) and NOT kept on the host -- the load paths
        # (adapters.load_embeddings_bin / load_sqlite_embeddings) for corpora that should not exist twice.  serialize() /
        # get_embedding_at() copy the matrix back on first use, after which the host copy is authoritative again.
        if keep_host_copy is None:
            keep_host_copy = os.environ.get("TYPEAGENT_VB_HOST_COPY", "1") not in ("0", "false", "no")
        self._keep_host = bool(keep_host_copy) or bool(self._devices)
        if corpus_dtype is None:
            self._dtype = _env_dtype()
        else:
            self._dtype = _native.TAVB_F16 if corpus_dtype.lower() in ("fp16", "f16", "half", "float16") else _native.TAVB_F32
        self._engine: _native.Engine | None = None
        self._host = np.zeros((0,), dtype=np.float32)  # backing store; _vectors is a view of its first _count rows
        self._count = 0
        self._dev_rows = 0  # rows of the host matrix already mirrored on the device
        self._dev_valid = True  # False => the device copy must be rebuilt from row 0
        # The live host matrix can be edited in place by whoever holds it (the reference always scores the live matrix, :176):
        #  * a matrix this index OWNS is handed out as a _WatchedMatrix view (`_watch` is its dirty flag);
        #  * a matrix the CALLER owns (deserialize(data) keeps `data` by reference, :287) cannot be wrapped: `_handed_out` turns on a
        #    fingerprint check per lookup -- "sampled" (default: 32 rows, ~30 us) or "full" (every byte: TYPEAGENT_VB_VERIFY_HOST=full /
        #    verify_host="full"; ~0.1 ms per MB) -- and mark_dirty() is the explicit form.
        self._watch = _Watch()
        self._view = None  # (host buffer, row count, the write-tracking view handed out for them)
        self._view_out = False  # a view of a matrix this index owns has been handed out: fingerprint fallback on (round-3 advice)
        self._handed_out = False
        self._dev_fingerprint = None
        self._fp_skipped = 0      # lookups since the fallback fingerprint of an owned, handed-out matrix was last compared
        self._fp_checked = 0.0    # ... and when (time.monotonic())
        mode = (verify_host or os.environ.get("TYPEAGENT_VB_VERIFY_HOST", "sampled")).lower()
        if mode not in ("sampled", "lazy", "full", "off"):
            raise ValueError("verify_host must be 'sampled', 'lazy', 'full' or 'off'")
        self._verify_host = mode
        self._device_only = None  # torch tensor when the corpus lives only on the device
        self._subset_cache = None  # (caller's subset object, private copy, row count, ordinals int64, device int32 rows) of the last subset lookup
        self._row_messages: np.ndarray | None = None  # chunk row -> message ordinal (message re-rank on the device)
        self._row_messages_rows = -1  # rows of the map already on the device
        self._removal_epoch = 0  # bumped by every remove_rows() / insert_rows() that changed a row's ordinal: a RowMask made before it names other rows now
        self._epoch_change = "removed from"  # what the last bump did ("removed from" / "inserted into"): the refusal says it
        self.clear()

    # ------------------------------------------------------------------ storage
    @property
    def _vectors(self) -> NormalizedEmbeddings:
        if self._device_only is not None:
            self._materialize_host()
        if self._handed_out:
            return self._host  # the caller's own matrix, adopted by reference: the same object every time (:271, :287)
        live = self._host
        cached = self._view
        if cached is not None and cached[0] is live and cached[1] == self._count:
            return cached[2]  # the same object for as long as the matrix is the same (the reference returns its one `_vectors`)
        if self._embedding_size > 0 and live.ndim == 2 and self._count != live.shape[0]:
            view = live[: self._count].view(_WatchedMatrix)  # the filled part of the growth buffer
        else:
            view = live.view(_WatchedMatrix)
        view._tavb_watch = self._watch
        self._view = (live, self._count, view)
        if not self._view_out:
            # from now on the lookups also keep the fingerprint of this matrix (writers the view cannot see); nobody has held a
            # view until now, so the mirror -- if there is one -- matches the matrix as it is
            self._view_out = True
            if self._dev_valid and self._dev_rows == self._count:
                self._dev_fingerprint = self._fingerprint()
        return view

    @_vectors.setter
    def _vectors(self, value: NormalizedEmbeddings) -> None:
        self._adopt_host(value)

    def _adopt_host(self, matrix: np.ndarray) -> None:
        self._device_only = None
        self._host = matrix
        self._count = len(matrix)
        self._dev_rows = 0
        self._dev_valid = False
        self._handed_out = True  # the caller keeps a reference to `matrix` (deserialize keeps it by reference, :287)
        other = getattr(matrix, "_tavb_watch", None)
        if other is not None and other is not self._watch and self._watch not in other.followers:
            other.followers.append(self._watch)  # another index's serialize() output: writes through it reach this index too

    def _materialize_host(self) -> None:
        t, n = self._device_only, self._count
        self._device_only = None
        if isinstance(t, list):
            host = np.concatenate([x.float().cpu().numpy() for x in t])[:n]
        else:
            host = t[:n].float().cpu().numpy()
        self._keep_host = True  # from here on the host matrix is the authoritative copy (like the reference's)
        self._host, self._count = host, n  # device copy stays valid: same rows (of an fp16 corpus the host copy holds the values widened to f32)

    def _reserve(self, extra: int) -> None:
        need = self._count + extra
        if self._host.ndim != 2 or self._host.shape[1] != self._embedding_size:
            self._host = np.zeros((max(need, 4), self._embedding_size), dtype=np.float32)
            self._handed_out = self._view_out = False
            return
        if need > self._host.shape[0] or self._handed_out:
            # (an adopted matrix is the caller's: appends go to a buffer of our own, like the reference's np.append copy, :128)
            if (self._handed_out or self._view_out) and self._dev_valid and self._dev_rows == self._count and self._dev_fingerprint != self._fingerprint():
                self._dev_valid = False  # edited in place since the last upload (also through a view the tracker cannot see): the rows already mirrored are stale too
            grown = np.empty((max(need, 2 * self._host.shape[0], 4), self._embedding_size), dtype=np.float32)
            grown[: self._count] = self._host[: self._count]
            self._host = grown
            self._handed_out = self._view_out = False  # (views of the old buffer are no longer views of this index' matrix)

    async def get_embedding(self, key: str, cache: bool = True) -> NormalizedEmbedding:
        if cache:
            return await self._model.get_embedding(key)
        return await self._model.get_embedding_nocache(key)

    async def get_embeddings(self, keys: list[str], cache: bool = True) -> NormalizedEmbeddings:
        if cache:
            return await self._model.get_embeddings(keys)
        return await self._model.get_embeddings_nocache(keys)

    def __len__(self) -> int:
        return self._count

    def __bool__(self) -> bool:  # an empty index is still truthy (:111-113)
        return True

    def add_embedding(self, key: str | None, embedding: NormalizedEmbedding | list[float]) -> None:
        row = np.asarray(embedding, dtype=np.float32)
        if self._embedding_size == 0:
            self._set_embedding_size(len(row))
        if len(row) != self._embedding_size:
            raise ValueError(f"Embedding size mismatch: expected {self._embedding_size}, got {len(row)}")
        if not self._stream_to_device(row.reshape(1, -1)):
            if self._device_only is not None:
                self._materialize_host()
            self._reserve(1)
            self._host[self._count] = row.reshape(-1)
            self._count += 1
        if key is not None:
            self._model.add_embedding(key, row)

    def add_embeddings(self, keys: None | list[str], embeddings: NormalizedEmbeddings) -> None:
        if embeddings.ndim != 2:
            raise ValueError(f"Expected 2D embeddings array, got {embeddings.ndim}D")
        if self._embedding_size == 0:
            self._set_embedding_size(embeddings.shape[1])
        if embeddings.shape[1] != self._embedding_size:
            raise ValueError(f"Embedding size mismatch: expected {self._embedding_size}, got {embeddings.shape[1]}")
        if not self._stream_to_device(embeddings):
            if self._device_only is not None:
                self._materialize_host()
            n = embeddings.shape[0]
            self._reserve(n)
            self._host[self._count : self._count + n] = embeddings
            self._count += n
        if keys is not None:
            for key, row in zip(keys, embeddings):
                self._model.add_embedding(key, row)

    def _stream_to_device(self, rows: np.ndarray) -> bool:
        """keep_host_copy=False: append `rows` to the device corpus only.  False when this index keeps its host matrix."""
        if self._keep_host or (self._count > 0 and self._device_only is None):
            return False  # (a host matrix already exists -- e.g. after serialize(): stay host-authoritative)
        eng = self._ensure_engine()
        if len(rows):
            eng.upload_rows(np.ascontiguousarray(rows, dtype=np.float32), self._count, self._dtype)
            self._count += len(rows)
            self._device_only = eng.corpus
            self._dev_rows, self._dev_valid = self._count, True
        return True

    async def add_key(self, key: str, cache: bool = True) -> None:
        embedding = await self.get_embedding(key, cache=cache)
        self.add_embedding(key if cache else None, embedding)

    async def add_keys(self, keys: list[str], cache: bool = True) -> NormalizedEmbeddings | None:
        if not keys:
            return None
        embeddings = await self.get_embeddings(keys, cache=cache)
        self.add_embeddings(keys if cache else None, embeddings)
        return embeddings

    # ------------------------------------------------------------------ device mirror
    def _ensure_engine(self) -> _native.Engine:
        if self._engine is None:
            if self._devices:
                from .multidevice import DeviceGroup

                self._engine = DeviceGroup(self._devices)
            else:
                self._engine = _native.Engine(self._device_index)
            level = os.environ.get("TYPEAGENT_VB_F32_SHADOW", "1").lower()
            if level in ("0", "false", "no"):
                self._engine.set_option("f32_shadow", 0)  # no fp16 shadow of fp32 corpora (+50 % device memory) for large batches
            elif level == "2":
                self._engine.set_option("f32_shadow", 2)  # every lookup on big fp32 corpora filters on the shadow (tavb.h)
        return self._engine

    def _sync_device(self) -> _native.Engine:
        eng = self._ensure_engine()
        if self._device_only is not None:
            return eng
        n = self._count
        if self._watch.dirty:  # a view handed out by serialize() / _vectors / get_embedding_at() was written to
            self._watch.dirty = False
            self._dev_valid = False
        if (self._handed_out or self._view_out) and self._dev_valid and self._dev_rows == n and n > 0 and self._fingerprint_due() \
                and self._dev_fingerprint != self._fingerprint():
            self._dev_valid = False  # the caller's matrix adopted by deserialize() -- or a matrix of ours somebody holds a view of -- was edited in place
        if not self._dev_valid:
            self._dev_rows = 0
            self._dev_valid = True
        if self._dev_rows > n:
            self._dev_rows = 0
        if self._dev_rows < n or eng.rows != n or eng.dim != self._embedding_size:
            start = self._dev_rows if (eng.corpus is not None and eng.dim == self._embedding_size and eng.dtype == self._dtype) else 0
            done = eng.upload_rows(self._host[start:n], start, self._dtype, capacity_hint=self._host.shape[0] if start == 0 else 0)
            if done is False:  # a device group has to re-shard: everything again
                eng.upload_rows(self._host[:n], 0, self._dtype, capacity_hint=self._host.shape[0])
            self._dev_rows = n
            self._dev_fingerprint = self._fingerprint() if (self._handed_out or self._view_out) else None
        return eng

    def _fingerprint_due(self) -> bool:
        """A matrix somebody else can write to -- the CALLER's own (deserialize(), :287), or one of ours that has been handed out as a view
        (serialize() / _vectors / get_embedding_at()) -- is fingerprinted before EVERY lookup (the reference always scores the live matrix,
        :176).  The view reports writers that use numpy's array API by itself; the fingerprint is what notices the others
        (torch.from_numpy on the view, ctypes, a C extension).  It costs as much as a whole lookup on a small corpus (~30 us), so
        `verify_host="lazy"` (opt-in) takes it for a matrix of ours at most once per 64 lookups or 20 ms, whichever comes first --
        such a writer may then be served stale answers for that long; `mark_dirty()` is the explicit, immediate form."""
        if self._handed_out or self._verify_host != "lazy":
            return True
        self._fp_skipped += 1
        now = time.monotonic()
        if self._fp_skipped >= 64 or now - self._fp_checked >= 0.02:
            self._fp_skipped = 0
            self._fp_checked = now
            return True
        return False

    def _fingerprint(self):
        """Watch on a matrix the CALLER owns (adopted by deserialize(), :287).  "sampled": hash of up to 32 evenly spaced rows
        (~30 us): whole-matrix edits (re-normalisation, bulk replacement) are caught, an edit confined to rows outside the
        sample is not.  "full": a 128-bit hash of every byte (xxh3, ~0.1 ms per MB on one core; blake2b when xxhash is not
        installed): nothing is missed, at a per-lookup cost that only small indexes can afford.  `mark_dirty()` is the explicit form."""
        n = self._count
        if n == 0 or self._host.ndim != 2 or self._verify_host == "off":
            return None
        if self._verify_host == "full":  # ("lazy" fingerprints like "sampled", less often: _fingerprint_due)
            data = memoryview(np.ascontiguousarray(self._host[:n])).cast("B")
            return (n, self._host.shape[1], _digest(data))
        idx = np.unique(np.linspace(0, n - 1, num=min(n, 32)).astype(np.int64))
        return hash((n, self._host.shape[1], self._host[idx].tobytes()))

    def mark_dirty(self) -> None:
        """Call after writing to the host matrix by a route numpy does not see (raw pointers, memoryview, a base-class view from
        np.asarray(serialize())), or -- for a matrix adopted by deserialize() under the default sampled watch -- after editing
        single rows of it: the device mirror is rebuilt on the next lookup."""
        self._dev_valid = False

    def adopt_device_corpus(self, tensor, rows: int | None = None, ordinal_base: int = 0) -> None:
        """Use a float32/float16 torch tensor [N, D] already on the GPU as the corpus
        without a host copy (corpora larger than host RAM).  serialize() will copy
        it back on demand.  With `devices=[...]`: a list of tensors, one row shard per device."""
        eng = self._ensure_engine()
        eng.ordinal_base = ordinal_base
        if self._devices:  # one tensor per device, row shards in order
            tensors = list(tensor) if isinstance(tensor, (list, tuple)) else [tensor]
            eng.set_shard_tensors(tensors, ordinal_base=ordinal_base)
            tensor = tensors
            self._set_embedding_size(int(tensors[0].shape[1]))
        else:
            eng.set_corpus_tensor(tensor, rows=rows, ordinal_base=ordinal_base)
            self._set_embedding_size(int(tensor.shape[1]))
        self._device_only = tensor
        self._count = eng.rows
        self._dtype = eng.dtype
        self._dev_rows, self._dev_valid = eng.rows, True
        self._host = np.zeros((0, self._embedding_size), dtype=np.float32)

    @property
    def engine(self) -> _native.Engine:
        """The device engine with the corpus synced (tuning knobs, profiling, device-resident calls)."""
        return self._sync_device()

    # ------------------------------------------------------------------ lookups
    @staticmethod
    def _limits(max_hits: int | None, min_score: float | None) -> tuple[int, np.float32]:
        if max_hits is None:
            max_hits = 10
        if min_score is None:
            min_score = 0.0
        if max_hits < 0:
            raise ValueError("max_hits must be >= 0")
        return max_hits, _native.f32_threshold(min_score)

    @staticmethod
    def _large_k(eng, max_hits: int) -> bool:
        """max_hits past the fused selection that the exact device top-k takes (tavb_search_topk): a single-GPU engine with the
        "large_k" option on (the default), or a device group all of whose engines are such engines (tavb_search_topk_device per shard,
        merged on the host); test doubles and "large_k" = 0 keep the emit-all route."""
        if not (_PAGE < max_hits <= _native.MAX_LARGE_K):
            return False
        if hasattr(eng, "large_k_capable"):  # multidevice.DeviceGroup
            return eng.large_k_capable()
        return isinstance(eng, _native.Engine) and eng.get_option("large_k") != 0

    @staticmethod
    def _sort_all(eng, max_hits: int) -> bool:
        """max_hits == 0 (every survivor) or past the large-k route, which the sorted device route takes (tavb_search_sorted): a
        single-GPU engine with the "sort_all" option on (the default); device groups and test doubles keep the emit-all route."""
        return (max_hits == 0 or max_hits > _native.MAX_LARGE_K) and isinstance(eng, _native.Engine) and eng.get_option("sort_all") != 0

    def _batch_args(self, embeddings, max_hits: int | None, min_score):
        """(queries float32 [Q, dim], max_hits, float32 threshold(s), the caller's thresholds per query or None) of a batch lookup;
        `min_score` may be a sequence with one threshold per query."""
        queries = np.asarray(embeddings, dtype=np.float32)
        if queries.ndim != 2:
            raise ValueError(f"Expected 2D embeddings array, got {queries.ndim}D")
        if min_score is not None and not np.isscalar(min_score) and np.ndim(min_score) == 1:
            # one threshold per query (Q calls of the reference have Q `min_score` arguments, :163-173): same kernels as a uniform batch
            if len(min_score) != len(queries):
                raise ValueError(f"Number of thresholds {len(min_score)} does not match number of embeddings {len(queries)}")
            per_query = list(min_score)
            max_hits, _ = self._limits(max_hits, 0.0)
            return queries, max_hits, np.asarray([_native.f32_threshold(0.0 if m is None else m) for m in per_query], dtype=np.float32), per_query
        max_hits, thr = self._limits(max_hits, min_score)
        return queries, max_hits, thr, None

    @staticmethod
    def _batch_of_one(embedding) -> np.ndarray:
        q = np.asarray(embedding, dtype=np.float32)
        if q.ndim != 1:
            raise ValueError(f"Expected 1D embedding, got {q.ndim}D")
        return q.reshape(1, -1)

    @staticmethod
    def _wrap_subset(ordinals, n: int) -> tuple[np.ndarray, np.ndarray]:
        """The caller's ordinals -> (they as int64 [S], the corpus rows they name), wrapped and range-checked as numpy indexes an array of n rows."""
        subset = np.asarray(ordinals)
        if subset.dtype.kind not in "iu":
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        subset = subset.astype(np.int64, copy=False).reshape(-1)
        rows = np.where(subset < 0, subset + n, subset)  # numpy index wrap (:218)
        bad = (rows < 0) | (rows >= n)
        if bad.any():
            raise IndexError(f"index {int(subset[np.argmax(bad)])} is out of bounds for axis 0 with size {n}")
        return subset, rows

    @staticmethod
    def _empty_batch(nq: int, max_hits: int, as_arrays: bool):
        if as_arrays:
            return np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32), np.zeros(nq, np.int32)
        return [[] for _ in range(nq)]

    @staticmethod
    def _batch_result(ords, scs, cnts, max_hits: int, as_arrays: bool, base: int = 0):
        """[Q, max_hits] result arrays -> what a batch lookup returns; `base`: the engine's ordinal_base where its ordinals carry it."""
        if base:
            ords -= base  # (rows of THIS index, as the subset lookup reports them)
        if as_arrays:
            return ords, scs, cnts
        return _scored_lists(ords, scs, cnts, max_hits)

    @staticmethod
    def _accept_array(acc: np.ndarray | None) -> np.ndarray | None:
        """int64 message ordinals -> those the device's int32 map can name (None: no filter)."""
        return None if acc is None else acc[(acc >= 0) & (acc < 2**31 - 1)]

    def fuzzy_lookup_embedding(
        self,
        embedding: NormalizedEmbedding,
        max_hits: int | None = None,
        min_score: float | None = None,
        predicate: Callable[[int], bool] | None = None,
    ) -> list[ScoredInt]:
        max_hits, thr = self._limits(max_hits, min_score)
        if self._count == 0:
            return []
        eng = self._sync_device()
        if predicate is None:
            if 1 <= max_hits <= _PAGE:
                ids, scs = eng.search(embedding, max_hits, thr)  # fused select-while-streaming
            elif self._large_k(eng, max_hits):
                ords, scs2, cnts = eng.search_topk(eng._query(embedding).reshape(1, -1), max_hits, thr)  # one pass, exact top-k on the device
                m = int(cnts[0])
                ids, scs = ords[0, :m], scs2[0, :m]
            elif self._sort_all(eng, max_hits):  # one pass, every survivor (or the best max_hits) sorted on the device
                ords, scs2, cnts = eng.search_sorted(eng._query(embedding).reshape(1, -1), max_hits, thr)
                return _sorted_lists(ords, scs2, cnts)[0]
            else:
                # more hits than the fused selection holds, or max_hits == 0 (every survivor, sorted: the `[-0:]` quirk,
                # :186-187): ONE pass emits all survivors, the host sorts them
                ids, scs = eng.search_all(embedding, thr, None if max_hits == 0 else max_hits)
            return list(map(ScoredInt, ids.tolist(), scs.tolist()))  # (tolist() yields Python ints / floats: the float32 scores widened, as the reference's float(score))
        # predicate path (:191-201): threshold on the device (one pass, all survivors), then exactly the reference's steps:
        # predicate(ordinal) for EVERY survivor in ascending ordinal order, stable sort by score, cut
        ids, scs = eng.search_all(embedding, thr, None)
        order = np.lexsort((ids,))  # ascending ordinal: the order of np.flatnonzero (:193)
        kept = [ScoredInt(int(i), float(s)) for i, s in zip(ids[order].tolist(), scs[order].tolist()) if predicate(int(i))]
        kept.sort(key=lambda x: x.score, reverse=True)
        return kept[:max_hits]

    def fuzzy_lookup_embedding_in_subset(
        self,
        embedding: NormalizedEmbedding,
        ordinals_of_subset: list[int],
        max_hits: int | None = None,
        min_score: float | None = None,
    ) -> list[ScoredInt]:
        max_hits, thr = self._limits(max_hits, min_score)
        if len(ordinals_of_subset) == 0 or self._count == 0:
            return []
        n = self._count
        # The same subset again (the memory provider hands in one scope list per query term, storage/memory/messageindex.py:173-183;
        # tools/benchmark_vectorbase.py:133-163 one list for every round): its wrapped, range-checked row list stays on the device.
        # Recognised by identity AND content -- `==` on the caller's list against a private copy (identical int objects compare by
        # pointer: ~3 ns per ordinal, against ~30 ns to convert one), so a list edited in place since is simply a new subset.
        cached = self._subset_cache
        hit = (cached is not None and cached[0] is ordinals_of_subset and cached[2] == n and len(cached[1]) == len(ordinals_of_subset)
               and (np.array_equal(cached[1], ordinals_of_subset) if isinstance(ordinals_of_subset, np.ndarray) else cached[1] == ordinals_of_subset))
        if hit:
            subset, rows, dev_rows = cached[3], None, cached[4]
        else:
            (subset, rows), dev_rows = self._wrap_subset(ordinals_of_subset, n), None
        eng = self._sync_device()
        if 1 <= max_hits <= _PAGE and isinstance(eng, _native.Engine) and isinstance(ordinals_of_subset, (list, np.ndarray)):
            if dev_rows is None:
                dev_rows = eng.rows_to_device(rows)
                is_array = isinstance(ordinals_of_subset, np.ndarray)  # (then `subset` may be a view of the caller's array: keep a copy)
                keep = ordinals_of_subset.copy() if is_array else list(ordinals_of_subset)
                subset = subset.copy() if is_array else subset
                self._subset_cache = (ordinals_of_subset, keep, n, subset, dev_rows)
            pos, scs = eng.search_subset_resident(embedding, dev_rows, max_hits, thr)
        else:
            if rows is None:
                rows = self._wrap_subset(subset, n)[1]
            if 1 <= max_hits <= _PAGE:
                pos, scs = eng.search_subset(embedding, rows, max_hits, thr)
            elif self._large_k(eng, max_hits):
                pos, scs = eng.search_subset_topk(embedding, rows, max_hits, thr)
            elif self._sort_all(eng, max_hits):
                pos, scs = eng.search_subset_sorted(embedding, rows, max_hits, thr)
            else:
                pos, scs = eng.search_all(embedding, thr, None if max_hits == 0 else max_hits, subset_rows=rows)
        return list(map(ScoredInt, subset[pos].tolist(), scs.tolist()))  # (the caller's ordinals at the returned positions, :229)

    def fuzzy_lookup_embeddings(
        self,
        embeddings: NormalizedEmbeddings,
        max_hits: int | None = None,
        min_score: float | None = None,
        as_arrays: bool = False,
    ):
        """Batch form: equals [fuzzy_lookup_embedding(e, max_hits, min_score) for e in embeddings],
        served by one device submission (the reference loops, storage/memory/reltermsindex.py:320-332).
        `min_score` may be a sequence with one threshold per query.
        `as_arrays=True` (1 <= max_hits <= 256) returns (ordinals int64 [Q, max_hits], scores float32 [Q, max_hits], counts
        int32 [Q]) instead of Q lists of ScoredInt: building 32k Python objects takes as long as a third of the 1024-query
        lookup over 10M rows itself."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_hits, min_score)
        if as_arrays and not (1 <= max_hits <= _PAGE):
            raise ValueError(f"as_arrays needs 1 <= max_hits <= {_PAGE}")
        if self._count == 0 or len(queries) == 0:
            return self._empty_batch(len(queries), max_hits, as_arrays)
        if not (1 <= max_hits <= _PAGE):
            eng = self._sync_device()
            if self._large_k(eng, max_hits):  # ONE call: a corpus pass per 8 queries, each query's own threshold
                ords, scs, cnts = eng.search_topk(queries, max_hits, thr)
                return _scored_lists(ords, scs, cnts, max_hits)
            if self._sort_all(eng, max_hits):  # ONE call as well: every query's survivors (or best max_hits) sorted on the device
                ords, scs, cnts = eng.search_sorted(queries, max_hits, thr)
                return _sorted_lists(ords, scs, cnts)
            return [self.fuzzy_lookup_embedding(q, max_hits, min_score if per_query is None else per_query[i]) for i, q in enumerate(queries)]
        eng = self._sync_device()
        return self._batch_result(*eng.search_batch(queries, max_hits, thr), max_hits, as_arrays)

    # ------------------------------------------------------------------ rows of the index as queries (additive)
    @staticmethod
    def _rows_native(eng) -> bool:
        """A single-GPU engine with the "rows_query" option on (the default) takes tavb_search_rows; device groups, test doubles and
        "rows_query" = 0 take the host route."""
        return isinstance(eng, _native.Engine) and hasattr(eng, "search_rows") and eng.get_option("rows_query") != 0

    def _rows_as_queries(self, pos: np.ndarray) -> np.ndarray:
        """Host route: rows `pos` as the float32 values the kernels multiply -- the host matrix' rows, through float16 where the corpus is
        stored as fp16 (the conversion the load path applies: round to nearest even)."""
        if self._device_only is not None:
            self._materialize_host()
        rows = np.ascontiguousarray(self._host[: self._count][pos], dtype=np.float32)
        if self._dtype == _native.TAVB_F16:
            with np.errstate(over="ignore"):
                rows = rows.astype(np.float16).astype(np.float32)
        return rows

    def _lookup_rows_arrays(self, eng, pos: np.ndarray, k: int, thr, exclude_self: bool, native: bool):
        """1 <= k: the best k neighbours of rows `pos` -> (ordinals [n, k] carrying the engine's ordinal base, scores [n, k], counts [n]).
        native: ONE call of tavb_search_rows.  Host route, the definition: the rows as a float32 query batch through
        `fuzzy_lookup_embeddings` with one hit more, the row's own entry removed, the first k kept."""
        if native:
            return eng.search_rows(pos, k, thr, exclude_self)
        queries = self._rows_as_queries(pos)
        kk = k + (1 if exclude_self else 0)
        if kk <= _PAGE:
            ords, scs, cnts = self.fuzzy_lookup_embeddings(queries, kk, thr, as_arrays=True)
        else:
            ords, scs, cnts = self._lists_as_rows(self.fuzzy_lookup_embeddings(queries, kk, thr), kk)
        if not exclude_self:
            return ords, scs, cnts
        own = pos + int(getattr(eng, "ordinal_base", 0))
        slot = np.arange(k + 1)[None, :]
        is_self = (ords == own[:, None]) & (slot < cnts[:, None])
        self_slot = np.where(is_self.any(axis=1), is_self.argmax(axis=1), k + 1)
        src = np.arange(k)[None, :] + (np.arange(k)[None, :] >= self_slot[:, None])
        out_cnts = np.minimum(cnts - is_self.any(axis=1), k).astype(np.int32)
        return np.take_along_axis(ords, src, axis=1), np.take_along_axis(scs, src, axis=1), out_cnts

    @staticmethod
    def _lists_as_rows(lists, k: int):
        """Q lists of ScoredInt -> (ordinals int64 [Q, k], float32 scores [Q, k], counts int32 [Q]), zero-padded."""
        ords = np.zeros((len(lists), k), np.int64)
        scs = np.zeros((len(lists), k), np.float32)
        cnts = np.zeros(len(lists), np.int32)
        for i, hits in enumerate(lists):
            m = len(hits)
            ords[i, :m] = [h.item for h in hits]
            scs[i, :m] = [h.score for h in hits]
            cnts[i] = m
        return ords, scs, cnts

    def fuzzy_lookup_rows(
        self,
        ordinals,
        max_hits: int | None = None,
        min_score: float | None = None,
        exclude_self: bool = True,
    ) -> list[list[ScoredInt]]:
        """The nearest neighbours of rows ALREADY in the index ("more like this"): per ordinal what
        `fuzzy_lookup_embedding(row, max_hits + 1, min_score)` returns with the row's own entry removed, cut to max_hits -- exactly, ties
        included.  `ordinals` index the rows as numpy would (negatives wrap, out of range raises IndexError, duplicates are answered
        twice; an int is a list of one).  exclude_self=False: the plain lookup with the rows as queries.  On a single-GPU engine the rows
        never leave the device (tavb_search_rows: gather, lookup, the own row dropped, one copy back); device groups, host-only doubles and
        the option "rows_query" = 0 take the host route, which is the definition and gives the same lists."""
        max_hits, thr = self._limits(max_hits, min_score)
        if isinstance(ordinals, (int, np.integer)):
            ordinals = [int(ordinals)]
        if len(ordinals) == 0:
            return []
        _, pos = self._wrap_subset(ordinals, self._count)  # (an empty index: every ordinal is out of range)
        eng = self._sync_device()
        native = self._rows_native(eng)
        extra = 1 if exclude_self else 0
        if 1 <= max_hits <= _native.MAX_LARGE_K - extra:
            ords, scs, cnts = self._lookup_rows_arrays(eng, pos, max_hits, thr, exclude_self, native)
            return _scored_lists(np.ascontiguousarray(ords), np.ascontiguousarray(scs), np.ascontiguousarray(cnts, dtype=np.int32), max_hits)
        if native and max_hits == 0 and eng.get_option("sort_all") != 0:  # every survivor: the sorted route, the own row dropped after the copy
            return _sorted_lists(*eng.search_rows_sorted(pos, thr, exclude_self))
        # every survivor (max_hits == 0) and max_hits beyond the large-k route, or engines without it: the plain lookups, the own entry removed by hand
        lists = self.fuzzy_lookup_embeddings(self._rows_as_queries(pos), max_hits + extra if max_hits else 0, thr)
        if not exclude_self:
            return lists
        own = (pos + int(getattr(eng, "ordinal_base", 0))).tolist()
        out = []
        for o, hits in zip(own, lists):
            at = next((i for i, h in enumerate(hits) if h.item == o), None)
            if at is not None:
                hits = hits[:at] + hits[at + 1:]
            out.append(hits[:max_hits] if max_hits else hits)
        return out

    def near_duplicate_pairs(self, min_score: float, max_per_row: int = 16, among=None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Near-duplicate detection: (i, j, score) with i < j, one entry per unordered pair -- for every row i (of `among`, a `RowMask`
        or anything `row_mask` takes, where given) the max_per_row best rows j > i (of `among`) scoring at least min_score; sorted by
        (i, score descending, j ascending).

        On a single-GPU engine whose index `tavb_plan_pairs_join` takes (option "pairs_join"; rows of a multiple of 64 elements, at least
        "pairs_join_min_rows" of them) the pairs come from ONE triangular self-join on the matrix cores (`similarity_join`), sorted and cut
        here without a per-row loop.  Everywhere else -- device groups, row shards, host-only doubles, a join that refused -- the rows are
        looked up in waves of the engine's "rows_query_wave" through the UNRESTRICTED lookup (`fuzzy_lookup_rows`' arrays):
        a wave asks for k best others per row; a row is settled when its list is not full (it holds every survivor) or holds
        max_per_row admissible j -- the admissible entries of the k best overall, in order, are the best admissible ones -- and the rows
        that are not are asked again with four times the k, at last for every survivor.  Nothing is approximated."""
        if max_per_row < 1:
            raise ValueError("max_per_row must be >= 1")
        _, thr = self._limits(1, min_score)
        n = self._count
        empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
        if n == 0:
            return empty
        joined = self._join_pairs_native(thr, among)
        if joined is not None:  # the self-join: the same pairs by definition -- every admissible pair, ordered, each row's run cut
            return self._order_pairs(*joined, max_per_row)
        allowed = None if among is None else self._mask_bools(self._resolve_mask(among))
        rows = np.arange(n, dtype=np.int64) if allowed is None else np.flatnonzero(allowed).astype(np.int64)
        rows = rows[rows < n - 1]  # (the last row has no j > i)
        if len(rows) == 0:
            return empty
        eng = self._sync_device()
        native = self._rows_native(eng)
        base = int(getattr(eng, "ordinal_base", 0))
        wave = int(eng.get_option("rows_query_wave")) if native else 4096
        k_max = min(_native.MAX_LARGE_K - 1, max(n - 1, 1))  # (n - 1: every other row)
        out_i, out_j, out_s = [], [], []

        def admit(i: int, js: np.ndarray, ss: np.ndarray):
            ok = js > i
            if allowed is not None:
                ok &= allowed[js]
            return js[ok], ss[ok]

        def settle(i: int, js: np.ndarray, ss: np.ndarray) -> None:
            js, ss = js[:max_per_row], ss[:max_per_row]
            out_i.append(np.full(len(js), i, np.int64))
            out_j.append(js)
            out_s.append(ss)

        for w0 in range(0, len(rows), wave):
            todo = rows[w0:w0 + wave]
            k = min(max_per_row + 1, k_max)
            done: dict[int, tuple] = {}
            while len(todo):
                ords, scs, cnts = self._lookup_rows_arrays(eng, todo, k, thr, True, native)
                again = []
                for r, i in enumerate(todo.tolist()):
                    m = int(cnts[r])
                    js, ss = admit(i, ords[r, :m] - base, scs[r, :m])
                    if m < k or k >= n - 1 or len(js) >= max_per_row:
                        done[i] = (js, ss)
                    else:
                        again.append(i)
                todo = np.asarray(again, dtype=np.int64)
                if len(todo) and k == k_max:  # every survivor of the rows still open
                    for i, hits in zip(todo.tolist(), self.fuzzy_lookup_rows(todo, 0, min_score)):
                        done[i] = admit(i, np.asarray([h.item for h in hits], np.int64) - base, np.asarray([h.score for h in hits], np.float32))
                    break
                k = min(4 * k, k_max)
            for i in rows[w0:w0 + wave].tolist():
                settle(i, *done[i])
        return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_s).astype(np.float32)

    def _join_pairs_native(self, thr, among):
        """The self-join where it serves this index (a single-GPU engine, `Engine.plans_pairs_join`, a mask held on the device) ->
        (i, j, scores) in arbitrary order, positions without the engine's ordinal base; None: the caller takes the row lookups."""
        eng = self._sync_device()
        if not (isinstance(eng, _native.Engine) and hasattr(eng, "join_pairs") and eng.plans_pairs_join()):
            return None
        dev_bits = None
        if among is not None:
            dev_bits = self._resolve_mask(among).dev_bits
            if dev_bits is None:
                return None
        got = eng.join_pairs(thr, dev_bits)
        if got is None:
            return None
        base = int(getattr(eng, "ordinal_base", 0))
        return got[0] - base, got[1] - base, got[2]

    @staticmethod
    def _order_pairs(i: np.ndarray, j: np.ndarray, s: np.ndarray, max_per_row: int | None):
        """Pairs in any order -> sorted by (i, score descending, j ascending), every row's run cut to its first max_per_row (None: whole)."""
        i, j, s = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(s, np.float32)
        order = np.lexsort((j, -s, i))
        i, j, s = i[order], j[order], s[order]
        if max_per_row is not None and len(i):
            at = np.arange(len(i))
            start = np.maximum.accumulate(np.where(np.concatenate([[True], i[1:] != i[:-1]]), at, 0))  # where each row's run begins
            keep = at - start < max_per_row
            i, j, s = i[keep], j[keep], s[keep]
        return i, j, s

    def similarity_join(self, min_score: float, among=None, max_per_row: int | None = None) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The self-join of the index: EVERY pair (i, j, score) with i < j (both in `among`, a `RowMask` or anything `row_mask` takes, where
        given) scoring at least min_score, sorted by (i, score descending, j ascending); max_per_row cuts every row's run to its best
        max_per_row.  A pair's score is what `fuzzy_lookup_embedding(row i, 0, min_score)` reports for row j.

        A single-GPU engine computes only the upper triangle of the rows' product on the matrix cores, tests the threshold there and
        scores exactly the few pairs that pass (tavb_join_pairs; `tavb_plan_pairs_join` and the option "pairs_join" decide).  Device
        groups, row shards, host-only doubles, rows that are no multiple of 64 elements, a corpus with a non-finite row and a result beyond
        "pairs_join_max_capacity" candidates take the row lookups: `near_duplicate_pairs`' route, every survivor per row for
        max_per_row=None."""
        if max_per_row is not None:
            return self.near_duplicate_pairs(min_score, max_per_row, among)
        _, thr = self._limits(1, min_score)
        n = self._count
        empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32))
        if n == 0:
            return empty
        joined = self._join_pairs_native(thr, among)
        if joined is not None:
            return self._order_pairs(*joined, None)
        allowed = None if among is None else self._mask_bools(self._resolve_mask(among))
        rows = np.arange(n, dtype=np.int64) if allowed is None else np.flatnonzero(allowed).astype(np.int64)
        rows = rows[rows < n - 1]
        if len(rows) == 0:
            return empty
        base = int(getattr(self._sync_device(), "ordinal_base", 0))
        out_i, out_j, out_s = [], [], []
        for w0 in range(0, len(rows), 4096):  # every survivor of every row, the admissible ones kept in the lookup's order
            todo = rows[w0:w0 + 4096]
            for i, hits in zip(todo.tolist(), self.fuzzy_lookup_rows(todo, 0, min_score)):
                js = np.asarray([h.item for h in hits], np.int64) - base
                ok = js > i
                if allowed is not None:
                    ok &= allowed[js]
                out_i.append(np.full(int(ok.sum()), i, np.int64))
                out_j.append(js[ok])
                out_s.append(np.asarray([h.score for h in hits], np.float32)[ok])
        return np.concatenate(out_i), np.concatenate(out_j), np.concatenate(out_s).astype(np.float32)

    # ------------------------------------------------------------------ masked lookups (additive)
    def row_mask(self, allowed) -> RowMask:
        """An allow-mask -- a bool array or sequence of length len(self), or a torch bool tensor (on the engine's device it never visits the
        host) -- expanded once into a `RowMask` that the masked lookups take in place of the mask.  The handle is tied to this index at this
        length."""
        n = self._count
        if _is_tensor(allowed):
            if "bool" not in str(allowed.dtype):
                raise TypeError(f"a mask must be bool, got {allowed.dtype}")
            if allowed.dim() != 1 or allowed.shape[0] != n:
                raise ValueError(f"mask covers {allowed.shape[0] if allowed.dim() else 0} rows, the index has {n}")
            eng = self._sync_device() if n else None
            if self._masked_native(eng) and allowed.is_cuda and (allowed.device.index or 0) == eng.device:
                return self._native_row_mask(eng, allowed, n)
            if self._masked_group(eng):  # a tensor on any device: every shard's slice goes to that shard's device
                shards, count, bounds = eng.mask_to_rows(allowed)
                return RowMask(self, n, count, shards=shards, bounds=bounds)
            allowed = allowed.cpu().numpy()
        a = np.asarray(allowed)
        if a.dtype != np.bool_:
            raise TypeError(f"a mask must be bool, got {a.dtype}")
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"mask covers {a.shape[0] if a.ndim else 0} rows, the index has {n}")
        if n == 0:
            return RowMask(self, 0, 0, flat=np.zeros(0, np.int64))
        eng = self._sync_device()
        if self._masked_native(eng):
            return self._native_row_mask(eng, a, n)
        if self._masked_group(eng):
            shards, count, bounds = eng.mask_to_rows(a)
            return RowMask(self, n, count, shards=shards, bounds=bounds)
        flat = np.flatnonzero(a)  # groups of test doubles, test doubles: the fallback's ordinal list
        return RowMask(self, n, len(flat), flat=flat)

    def _native_row_mask(self, eng, allowed, n: int) -> RowMask:
        if hasattr(eng, "mask_to_rows_bits"):  # the packed mask stays on the device next to the row list: the tile route reads it
            dev_rows, count, dev_bits = eng.mask_to_rows_bits(allowed)
            return RowMask(self, n, count, dev_rows=dev_rows, dev_bits=dev_bits)
        dev_rows, count = eng.mask_to_rows(allowed)
        return RowMask(self, n, count, dev_rows=dev_rows)

    @staticmethod
    def _mask_plan(eng, mask: RowMask, nq: int, k: int, wide: bool) -> bool:
        """`_mask_tile` (wide=False) / `_mask_wide`: the engine has the call, the handle what the route reads, and the route's option
        (0 = never, 2 = wherever the route serves the shape, 1 = where its plan function expects it to win) says so.  The answer is kept on the handle."""
        call, plan, option, probe_nq, prefix = (("search_masked_wide", "plan_masked_wide", "mask_wide", _native.MFMA_MIN_BATCH, ("wide",)) if wide else
                                                ("search_masked_batch", "plan_masked", "mask_tile", 64, ()))
        if mask.dev_bits is None or mask.span is None or (wide and mask.dev_rows is None) or not (hasattr(eng, call) and hasattr(eng, plan)):
            return False
        cached = option + "_options"
        opts = getattr(eng, cached)() if hasattr(eng, cached) else tuple(eng.get_option(n) for n in (option, "mask_tile_min_bytes", "mask_tile_pct"))
        mode, min_bytes, pct = opts
        if mode == 0:
            return False
        key = prefix + (nq, k, eng.dim, eng.dtype, opts)
        yes = mask._plans.get(key)
        if yes is None:
            if mode == 2:
                # (tile: 64 queries, wide: the fewest queries the rule takes; one allowed row in a span of one, no floors: the rule says yes
                # exactly when the route serves the corpus, k and the width)
                yes = bool(getattr(eng, plan)(probe_nq, k, eng.dim, eng.dtype, 1, 1, 0, 0))
            else:
                yes = bool(getattr(eng, plan)(nq, k, eng.dim, eng.dtype, mask.count, mask.span[1] + 1 - mask.span[0] // 256 * 256, min_bytes, pct))
            mask._plans[key] = yes
        return yes

    @classmethod
    def _mask_tile(cls, eng, mask: RowMask, nq: int, k: int) -> bool:
        """Whether a masked batch takes the 32/64-query tile (Engine.search_masked_batch) instead of the gather route: the engine has the
        call, the handle the packed mask, and the option "mask_tile" (0 = never, 2 = wherever the tile serves the shape, 1 = where
        tavb_plan_masked expects it to win: a dense mask under a real batch) says so."""
        return cls._mask_plan(eng, mask, nq, k, wide=False)

    @classmethod
    def _mask_wide(cls, eng, mask: RowMask, nq: int, k: int) -> bool:
        """Whether a masked batch takes the 128/256-query filter tile + rescoring (Engine.search_masked_wide): the engine has the call, the
        handle the packed mask and the row list, and the option "mask_wide" (0 = never, 2 = wherever the route serves the shape, 1 = where
        tavb_plan_masked_wide expects it to win) says so.  The plan is kept on the handle like `_mask_tile`'s."""
        return cls._mask_plan(eng, mask, nq, k, wide=True)

    @classmethod
    def _masked_route(cls, eng, mask: RowMask, nq: int, k: int) -> int:
        """The route of a masked batch of k >= 1 hits on a single-GPU engine, as "masked_route" numbers them: 3 = the 128/256-query filter
        tile + rescoring (k <= 256; tried first), 2 = the 32/64-query tile (k <= 64), 1 = the row list."""
        if k <= _PAGE and cls._mask_wide(eng, mask, nq, k):
            return 3
        if k <= 64 and cls._mask_tile(eng, mask, nq, k):
            return 2
        return 1

    @staticmethod
    def _masked_native(eng) -> bool:
        """A single-GPU engine that expands masks and searches their row list itself (tavb_mask_expand, tavb_search_subset_batch_resident);
        device groups and test doubles take the fallback."""
        return isinstance(eng, _native.Engine) and hasattr(eng, "mask_to_rows") and hasattr(eng, "search_subset_batch_resident")

    @staticmethod
    def _masked_group(eng) -> bool:
        """A device group all of whose engines expand masks and search their row list themselves (multidevice.DeviceGroup.search_masked:
        tavb_mask_expand and tavb_search_subset_batch_device per shard); groups of test doubles take the fallback."""
        return eng is not None and hasattr(eng, "masked_capable") and eng.masked_capable()

    def _resolve_mask(self, allowed) -> RowMask:
        if not isinstance(allowed, RowMask):
            return self.row_mask(allowed)
        if allowed._owner() is not self:
            raise ValueError("this RowMask was built by another index")
        if allowed.rows != self._count:
            raise ValueError(f"mask covers {allowed.rows} rows, the index has {self._count}")
        if allowed.epoch != self._removal_epoch:
            raise ValueError(f"this RowMask was built before rows were {self._epoch_change} the index: build it again")
        return allowed

    # ------------------------------------------------------------------ scope algebra (additive)
    def _mask_bools(self, mask: RowMask) -> np.ndarray:
        b = np.zeros(self._count, dtype=bool)
        b[mask.flat()] = True
        return b

    def _combine_masks(self, op: int, masks) -> RowMask:
        """AND / OR of any number of masks, or ANDNOT (the first without the others; one operand: its complement) of up to 8 -- `RowMask`s of
        this index at this length, or anything `row_mask` takes.  On a single-GPU engine operands that hold their packed mask on the device
        are combined there, up to 8 per launch (tavb_mask_combine; more are folded in groups), and the result is a full handle; everywhere
        else the bool arrays are combined on the host and handed to `row_mask`."""
        handles = [self._resolve_mask(m) for m in masks]
        if not handles:
            raise ValueError("at least one mask is needed")
        n = self._count
        if n == 0:
            return RowMask(self, 0, 0, flat=np.zeros(0, np.int64))
        eng = self._sync_device()
        if self._masked_native(eng) and hasattr(eng, "mask_combine") and all(h.dev_bits is not None for h in handles):
            most = _native.MAX_MASK_OPERANDS
            if op == _native.MASK_ANDNOT and len(handles) > most:  # a \ (b | c | ...): the union first
                handles = [handles[0], self._combine_masks(_native.MASK_OR, handles[1:])]
            while True:
                group, handles = handles[:most], handles[most:]
                counts = [h.count for h in group]
                if op == _native.MASK_AND:
                    cap = min(counts)
                elif op == _native.MASK_OR:
                    cap = min(sum(counts), n)
                else:
                    cap = counts[0] if len(group) > 1 else n - counts[0]
                dev_rows, count, dev_bits, span = eng.mask_combine(op, [h.dev_bits for h in group], cap)
                out = RowMask(self, n, count, dev_rows=dev_rows, dev_bits=dev_bits, span=span)
                if not handles:
                    return out
                handles.insert(0, out)
        bools = [self._mask_bools(h) for h in handles]
        if op == _native.MASK_AND:
            return self.row_mask(np.logical_and.reduce(bools))
        if op == _native.MASK_OR:
            return self.row_mask(np.logical_or.reduce(bools))
        return self.row_mask(bools[0] & ~np.logical_or.reduce(bools[1:]) if len(bools) > 1 else ~bools[0])

    def intersect_masks(self, *masks) -> RowMask:
        """The rows every one of `masks` allows: equals row_mask(A & B & ...) of their bool arrays.  `a & b` on two handles is this."""
        return self._combine_masks(_native.MASK_AND, masks)

    def union_masks(self, *masks) -> RowMask:
        """The rows any of `masks` allows: equals row_mask(A | B | ...) of their bool arrays.  `a | b` on two handles is this; `a - b` is
        row_mask(A & ~B) and `~a` row_mask(~A)."""
        return self._combine_masks(_native.MASK_OR, masks)

    def range_mask(self, collections, of: str = "rows") -> RowMask:
        """The `RowMask` of a scope given as COLLECTIONS of half-open (start, end) ranges -- the reference's `TextRangesInScope`
        (knowpro/collections.py:486-562): a row is allowed when EVERY collection has a range that holds it.  of="rows": the ranges are
        over index positions, equals row_mask(np.logical_and.reduce([union of the collection's ranges as a bool array ...])); of="messages":
        over message ordinals, tested on the row's message (`set_row_messages`; rows without a message are never allowed).  No collection
        at all allows every row (every row with a message); a collection without a non-empty range allows none.  Ranges may be unsorted,
        overlapping, duplicated, empty, or reach outside the index.  On a single-GPU engine only the ranges travel (8 collections per
        launch of tavb_mask_from_ranges; more are intersected on the device); device groups and test doubles build the bool array on the
        host."""
        if of not in _native.SCOPE_DOMAINS:
            raise ValueError(f'of must be "rows" or "messages", got {of!r}')
        cols = _native.range_collections(collections)
        if of == "messages":
            self._check_row_messages()
        n = self._count
        if n == 0:
            return RowMask(self, 0, 0, flat=np.zeros(0, np.int64))
        eng = self._messages_engine() if of == "messages" else self._sync_device()
        if eng is not None and self._masked_native(eng) and hasattr(eng, "mask_from_ranges"):
            most = _native.MAX_SCOPE_COLLECTIONS
            parts = []
            for i in range(0, max(len(cols), 1), most):
                dev_rows, count, dev_bits, span = eng.mask_from_ranges(cols[i:i + most], of)
                parts.append(RowMask(self, n, count, dev_rows=dev_rows, dev_bits=dev_bits, span=span))
            return parts[0] if len(parts) == 1 else self.intersect_masks(*parts)
        if of == "rows":
            ok = np.ones(n, dtype=bool)
            for c in cols:
                ok &= _native.ranges_to_bool(c, n)
            return self.row_mask(ok)
        held = self._row_messages[:n]
        ok = held >= 0
        n_messages = int(held.max()) + 1 if ok.any() else 0
        for c in cols:
            ok &= np.isin(held, np.flatnonzero(_native.ranges_to_bool(c, n_messages)))
        return self.row_mask(ok)

    def fuzzy_lookup_embedding_masked(
        self,
        embedding: NormalizedEmbedding,
        allowed,
        max_hits: int | None = None,
        min_score: float | None = None,
    ) -> list[ScoredInt]:
        """`fuzzy_lookup_embedding` among the rows `allowed` names (a mask, see `row_mask`, or a `RowMask`): equals
        fuzzy_lookup_embedding_in_subset(embedding, np.flatnonzero(allowed).tolist(), max_hits, min_score)."""
        return self.fuzzy_lookup_embeddings_masked(self._batch_of_one(embedding), allowed, max_hits, min_score)[0]

    def fuzzy_lookup_embeddings_masked(
        self,
        embeddings: NormalizedEmbeddings,
        allowed,
        max_hits: int | None = None,
        min_score: float | None = None,
        as_arrays: bool = False,
    ):
        """Batch form over ONE mask: equals [fuzzy_lookup_embedding_in_subset(e, np.flatnonzero(allowed).tolist(), max_hits, min_score)
        for e in embeddings].  On a single-GPU engine with 1 <= max_hits <= 16384 (beyond 256: while the "large_k" option is on, as for
        every other lookup) it is one submission -- the queries go over the
        mask's resident row list eight per pass -- and with a `RowMask` only the queries travel; a device group does the same on every
        shard that has allowed rows (one batched call per shard, merged on the host).  max_hits == 0 and beyond 16384 are one submission
        on a single-GPU engine as well, on the device sort route over the same row list (tavb_search_subset_batch_sorted, while
        "sort_all" is on); everything else ("large_k" off beyond 256, "sort_all" off, max_hits == 0 or beyond 16384 on a device group,
        test doubles) loops over `fuzzy_lookup_embedding_in_subset`.  `min_score` may be a sequence with one
        threshold per query; `as_arrays=True` (1 <= max_hits <= 256) as in `fuzzy_lookup_embeddings`.

        A DENSE mask under a real batch (1 <= max_hits <= 64, rows of a multiple of 64 bytes; engine option "mask_tile": by default from
        128 MiB of allowed rows, where eight queries per pass over them move at least the bytes of 64 queries per pass over the mask's
        span) runs on the 32/64-query matrix-core tile instead: the span of the mask is read once per 64 queries and the mask's bit is
        tested where a row is admitted.  There a batch equals the sequential subset lookups the way `fuzzy_lookup_embeddings` on the same
        tile equals `fuzzy_lookup_embedding`: the ordinals are identical except among float32 near-ties and the scores agree within
        1e-5 -- it is not bit for bit.

        From 65 queries on an fp16 corpus (1 <= max_hits <= 256, any width; engine option "mask_wide": by default under the same 128 MiB
        and byte-parity rule, with the 128 or 256 queries per pass of that tile) a dense mask runs where every large unmasked batch runs: the
        128/256-query filter tile, the mask's bit tested where a row is admitted, and exact rescoring of its candidates.  It is tried before
        the 32/64-query tile, and its answers EQUAL the row list's bit for bit -- ordinals, float32 scores and counts -- because the
        rescoring is the streaming kernels' arithmetic; a query with more near-duplicates around its last hit than a candidate band holds is
        re-run over the row list.  `engine.get_option("masked_route")` tells which ran (1 = row list, 2 = 32/64-query tile, 3 = wide)."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_hits, min_score)
        if as_arrays and not (1 <= max_hits <= _PAGE):
            raise ValueError(f"as_arrays needs 1 <= max_hits <= {_PAGE}")
        mask = self._resolve_mask(allowed)
        nq = len(queries)
        if self._count == 0 or mask.count == 0 or nq == 0:
            return self._empty_batch(nq, max_hits, as_arrays)
        eng = self._sync_device()
        if self._masked_native(eng) and mask.dev_rows is not None and (1 <= max_hits <= _PAGE or self._large_k(eng, max_hits)):
            route = self._masked_route(eng, mask, nq, max_hits)
            if route == 3:
                out = eng.search_masked_wide(queries, mask.dev_bits, mask.dev_rows, max_hits, thr, span=mask.span)
            elif route == 2:
                out = eng.search_masked_batch(queries, mask.dev_bits, max_hits, thr, span=mask.span)
            else:
                out = eng.search_subset_batch_resident(queries, mask.dev_rows, max_hits, thr, remap=True)
            return self._batch_result(*out, max_hits, as_arrays, base=eng.ordinal_base)
        if self._masked_native(eng) and mask.dev_rows is not None and hasattr(eng, "search_subset_batch_sorted") and self._sort_all(eng, max_hits):
            ords, scs, cnts = eng.search_subset_batch_sorted(queries, mask.dev_rows, max_hits, thr)
            return _sorted_lists(ords - eng.ordinal_base, scs, cnts)
        if self._masked_group(eng) and mask.shards is not None and (1 <= max_hits <= _PAGE or self._large_k(eng, max_hits)):
            if mask.bounds != tuple(eng.bounds):
                # the same index at the same length under other shard bounds (grown row by row, then re-uploaded from row 0): the
                # caller has done nothing wrong -- the handle is cut again, once
                mask.shards, _, mask.bounds = eng._rows_to_handles(mask.flat())
            return self._batch_result(*eng.search_masked(queries, mask.shards, max_hits, thr), max_hits, as_arrays, base=eng.ordinal_base)
        flat = mask.flat()
        lists = [self.fuzzy_lookup_embedding_in_subset(q, flat, max_hits, min_score if per_query is None else per_query[i]) for i, q in enumerate(queries)]
        return self._lists_as_arrays(lists, max_hits) if as_arrays else lists

    @staticmethod
    def _lists_as_arrays(lists, max_hits: int):
        """Q lists of ScoredInt -> the (ordinals [Q, max_hits], scores [Q, max_hits], counts [Q]) form of `as_arrays=True`."""
        nq = len(lists)
        ords, scs = np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32)
        cnts = np.array([len(hits) for hits in lists], dtype=np.int32)
        for i, hits in enumerate(lists):
            ords[i, : len(hits)] = [h.item for h in hits]
            scs[i, : len(hits)] = [h.score for h in hits]
        return ords, scs, cnts

    # ------------------------------------------------------------------ scoped batches: one mask per query (additive)
    def _resolve_scopes(self, scopes, nq: int) -> list[RowMask]:
        """One scope per query -> their handles (`_resolve_mask` each; an object that appears several times is resolved once, so that its
        queries share a handle)."""
        scopes = list(scopes)
        if len(scopes) != nq:
            raise ValueError(f"Number of scopes {len(scopes)} does not match number of embeddings {nq}")
        seen: dict[int, RowMask] = {}
        handles = []
        for s in scopes:
            h = seen.get(id(s))
            if h is None:
                h = seen[id(s)] = self._resolve_mask(s)
            handles.append(h)
        return handles

    @staticmethod
    def _scoped_order(handles) -> list[int]:
        """The queries that have something to search, ordered so that identical handles sit next to each other (groups in the order of their
        first query, queries in the caller's order inside a group): queries of one scope share the passes of the native call, and a pass'
        union is then the fewest rows.  Empty scopes take no slot."""
        first: dict[int, int] = {}
        for i, h in enumerate(handles):
            first.setdefault(id(h), i)
        return sorted((i for i, h in enumerate(handles) if h.count > 0), key=lambda i: (first[id(handles[i])], i))

    @staticmethod
    def _scoped_native(eng, call: str, handles, order, max_hits: int) -> bool:
        """The native route of a scoped batch: a single-GPU engine that has `call`, 1 <= max_hits <= 256, and every searched scope holds its
        packed mask on the device."""
        return (isinstance(eng, _native.Engine) and hasattr(eng, call) and 1 <= max_hits <= _PAGE
                and all(handles[i].dev_bits is not None for i in order))

    @classmethod
    def _scoped_large(cls, eng, handles, order, max_hits: int):
        """The one-call route of a scoped batch beyond the fused selection, by the name of its Engine method, or None (the loop over the
        per-query masked lookups): "search_scoped_topk" for max_hits 257 .. 16384 where `_large_k` holds, "search_scoped_sorted" for
        max_hits == 0 and beyond 16384 where `_sort_all` holds -- on a single-GPU engine that has the call, with the option
        "scope_large_k" on and every searched scope holding its packed mask on the device."""
        call = ("search_scoped_topk" if cls._large_k(eng, max_hits) else
                "search_scoped_sorted" if cls._sort_all(eng, max_hits) else None)
        if call is None or not hasattr(eng, call) or any(handles[i].dev_bits is None for i in order):
            return None
        return call if eng.get_option("scope_large_k") != 0 else None

    @staticmethod
    def _scoped_tile(eng, call: str, handles, order, max_hits: int):
        """Whether a scoped batch the native route serves takes the 32/64-query tile (`call`: Engine.search_scoped_tile /
        search_messages_scoped_tile): max_hits <= 64, every searched handle knows its span, and the option "scope_tile" (0 = never, 2 =
        wherever the tile serves the shape, 1 = where tavb_plan_scoped expects it to win: dense scopes under a real batch) says so.
        Returns the span (first, last) of the union of the searched scopes, or None: the row-list route.  Decided once per call from the
        handles' counts and spans -- no device work, nothing kept."""
        if max_hits > 64 or not (hasattr(eng, call) and hasattr(eng, "plan_scoped")) or any(handles[i].span is None for i in order):
            return None
        opts = eng.scope_tile_options() if hasattr(eng, "scope_tile_options") else tuple(
            eng.get_option(n) for n in ("scope_tile", "mask_tile_min_bytes", "mask_tile_pct"))
        mode, min_bytes, pct = opts
        if mode == 0:
            return None
        first, last = min(handles[i].span[0] for i in order), max(handles[i].span[1] for i in order)
        if mode == 2:  # (64 queries, one row in a span of one, no floors: yes exactly when the tile serves the corpus, max_hits and the width)
            yes = eng.plan_scoped(64, max_hits, eng.dim, eng.dtype, 1, 1, 0, 0)
        else:
            gather = _native.scoped_gather_rows([handles[i].count for i in order])
            yes = eng.plan_scoped(len(order), max_hits, eng.dim, eng.dtype, gather, last + 1 - first // 256 * 256, min_bytes, pct)
        return (first, last) if yes else None

    @staticmethod
    def _scoped_wide(eng, call: str, handles, order, max_hits: int):
        """Whether a scoped batch the native route serves takes the 128/256-query filter tile + rescoring (`call`:
        Engine.search_scoped_wide / search_messages_scoped_wide) -- asked BEFORE `_scoped_tile`, over which it wins: every searched handle
        knows its span and the option "scope_wide" (0 = never, 2 = wherever the route serves the shape, 1 = where tavb_plan_scoped_wide
        expects it to win) says so.  An engine without the call or the plan (an older library, a test double) keeps its routes.  Returns
        the span (first, last) of the union of the searched scopes, or None."""
        if not (hasattr(eng, call) and hasattr(eng, "plan_scoped_wide")) or any(handles[i].span is None for i in order):
            return None
        opts = eng.scope_wide_options() if hasattr(eng, "scope_wide_options") else tuple(
            eng.get_option(n) for n in ("scope_wide", "mask_tile_min_bytes", "mask_tile_pct"))
        mode, min_bytes, pct = opts
        if mode == 0:
            return None
        first, last = min(handles[i].span[0] for i in order), max(handles[i].span[1] for i in order)
        if mode == 2:  # (128 queries, no floors: yes exactly when the route serves the corpus, max_hits and the width)
            yes = eng.plan_scoped_wide(128, max_hits, eng.dim, eng.dtype, 1, 1, 0, 0)
        else:
            gather = _native.scoped_gather_rows([handles[i].count for i in order], 4 if max_hits > 64 else 8)
            yes = eng.plan_scoped_wide(len(order), max_hits, eng.dim, eng.dtype, gather, last + 1 - first // 256 * 256, min_bytes, pct)
        return (first, last) if yes else None

    def fuzzy_lookup_embeddings_scoped(
        self,
        embeddings: NormalizedEmbeddings,
        scopes,
        max_hits: int | None = None,
        min_score: float | None = None,
        as_arrays: bool = False,
    ):
        """A batch whose queries carry their OWN scopes -- the lookups of one compiled question, each under its `when` filter: `scopes` is a
        sequence with one entry per query, each anything `fuzzy_lookup_embedding_masked` takes (a `RowMask` of this index, a bool array, a
        bool tensor).  Equals [fuzzy_lookup_embedding_masked(e, s, max_hits, min_score_i) for e, s in zip(embeddings, scopes)], and so
        fuzzy_lookup_embedding_in_subset(e, np.flatnonzero(s).tolist(), ...) per query.  `min_score` may be a sequence with one threshold per
        query; `as_arrays=True` (1 <= max_hits <= 256) as in `fuzzy_lookup_embeddings_masked`.  A different number of scopes and embeddings
        raises ValueError; a handle of another index, another length or from before an edit raises what the masked lookups raise.

        When every scope is the same handle this IS `fuzzy_lookup_embeddings_masked` over it.  Otherwise, on a single-GPU engine with 1 <=
        max_hits <= 256 whose scopes all hold their packed mask on the device (handles from `row_mask`, `range_mask`, `message_mask` and
        the scope algebra do), the batch is ONE submission (tavb_search_scoped_batch): the queries are ordered so that identical handles sit
        next to each other, go in passes of eight (four for max_hits > 64; fewer on rows so wide -- from about 4.7k floats -- that eight
        queries do not fit the vector tier's on-chip memory, so that a pass keeps the per-row arithmetic of a single query) over the UNION
        of the pass' scopes -- built, listed and tested on the device; a row several scopes share is read once per pass -- and the answers
        come back in the caller's order, bit for bit those of the per-query calls on the row list: ordinals, float32 scores and counts.
        Batches beyond 16 passes (128 queries) go in waves of that many, each with one wait for its unions' sizes, which bounds the
        device workspace whatever the batch.  A query whose scope is empty gets an empty answer
        and takes no slot.  `engine.get_option("masked_route")` is then 4.

        DENSE scopes under a real batch (1 <= max_hits <= 64, rows of a multiple of 64 bytes; engine option "scope_tile": by default where
        tavb_plan_scoped says so -- the row-list route would read at least 128 MiB per pass and at least as many rows as the tile) run on
        the 32/64-query matrix-core tile instead (tavb_search_scoped_tile): the span of the union of the scopes is read once per 64
        queries and each query's scope is tested in the tile's admission path.  The answers are then the TILE's -- those of
        `fuzzy_lookup_embeddings_masked` on its tile route: equal to the per-query calls except among float32 near-ties, scores within a
        few 1e-7, not bit for bit.  `engine.get_option("masked_route")` is then 5.

        From 65 queries on an fp16 corpus (any width, 1 <= max_hits <= 256; engine option "scope_wide": where tavb_plan_scoped_wide says
        so, and then in preference to the 32/64-query tile) dense scopes run on the 128/256-query filter tile with exact rescoring
        (tavb_search_scoped_wide): the span is read once per 128 or 256 queries, each query's scope is tested in the filter's admission
        path, and the candidates are scored again with the streaming kernels' arithmetic -- the answers of the row-list route BIT FOR
        BIT, at max_hits up to 256.  `engine.get_option("masked_route")` is then 6.

        Beyond 256 the batch stays ONE submission on a single-GPU engine whose scopes all hold their device mask (engine option
        "scope_large_k", default 1): max_hits 257 .. 16384 (while "large_k" is on) runs the exact device top-k under scopes
        (tavb_search_scoped_topk) and max_hits == 0 or beyond 16384 (while "sort_all" is on) the device sort (tavb_search_scoped_sorted:
        every survivor of the query's own scope, or its best max_hits) -- the same passes of eight queries over the union of their scopes,
        a row scored for a query only inside that query's scope, answers bit for bit those of the per-query calls.
        `engine.get_option("masked_route")` is then 7 and 8.

        Everything else loops over `fuzzy_lookup_embedding_masked`: "scope_large_k", "large_k" or "sort_all" switched off, device groups,
        `ShardedVectorBase`, `FusedIndexQuery`, test doubles, and a handle without a device mask; so does
        `lookup_messages_by_embeddings_scoped` at max_matches above 256.  The tile routes serve single-GPU engines only: device groups,
        `ShardedVectorBase` and `FusedIndexQuery` do not take them; max_hits 65 .. 256 is served on the 128/256-query tile only (fp16
        corpora), and queries are not reordered by how much their scopes overlap -- only identical handles are grouped."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_hits, min_score)
        if as_arrays and not (1 <= max_hits <= _PAGE):
            raise ValueError(f"as_arrays needs 1 <= max_hits <= {_PAGE}")
        nq = len(queries)
        handles = self._resolve_scopes(scopes, nq)
        if nq and all(h is handles[0] for h in handles):
            return self.fuzzy_lookup_embeddings_masked(queries, handles[0], max_hits, min_score if per_query is None else per_query, as_arrays)
        order = self._scoped_order(handles)
        if self._count == 0 or not order:
            return self._empty_batch(nq, max_hits, as_arrays)
        eng = self._sync_device()
        if self._scoped_native(eng, "search_scoped_batch", handles, order, max_hits):
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
            wide = self._scoped_wide(eng, "search_scoped_wide", handles, order, max_hits)
            span = None if wide is not None else self._scoped_tile(eng, "search_scoped_tile", handles, order, max_hits)
            if wide is not None:
                o, s, c = eng.search_scoped_wide(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                 np.ascontiguousarray(t[order]), span=wide)
            elif span is not None:
                o, s, c = eng.search_scoped_tile(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                 np.ascontiguousarray(t[order]), span=span)
            else:
                o, s, c = eng.search_scoped_batch(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                  np.ascontiguousarray(t[order]))
            ords, scs, cnts = np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32), np.zeros(nq, np.int32)
            ords[order], scs[order], cnts[order] = o - eng.ordinal_base, s, c
            return (ords, scs, cnts) if as_arrays else _scored_lists(ords, scs, cnts, max_hits)
        large = self._scoped_large(eng, handles, order, max_hits)
        if large is not None:
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
            sub_q, sub_t, masks = np.ascontiguousarray(queries[order]), np.ascontiguousarray(t[order]), [handles[i].dev_bits for i in order]
            if large == "search_scoped_topk":
                o, s, c = eng.search_scoped_topk(sub_q, masks, max_hits, sub_t)
                ords, scs, cnts = np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32), np.zeros(nq, np.int32)
                ords[order], scs[order], cnts[order] = o - eng.ordinal_base, s, c
                return _scored_lists(ords, scs, cnts, max_hits)
            bound = sum(handles[i].count if max_hits == 0 else min(max_hits, handles[i].count) for i in order)
            o, s, c = eng.search_scoped_sorted(sub_q, masks, max_hits, sub_t, bound)
            lists = [[] for _ in range(nq)]
            for i, hits in zip(order, _sorted_lists(o - eng.ordinal_base, s, c)):
                lists[i] = hits
            return lists
        lists = [self.fuzzy_lookup_embedding_masked(q, handles[i], max_hits, min_score if per_query is None else per_query[i]) for i, q in enumerate(queries)]
        return self._lists_as_arrays(lists, max_hits) if as_arrays else lists

    # ------------------------------------------------------------------ message re-rank (additive)
    def set_row_messages(self, row_to_message) -> None:
        """chunk row -> message ordinal for every row of the index (-1: none): what the providers keep as
        `TextLocation.message_ordinal` per index position (knowpro/textlocindex.py:54-73; the `msg_id` column of
        storage/sqlite/schema.py:71-81).  Enables `lookup_messages_by_embedding*`, which run the providers' post-lookup
        aggregation on the device."""
        self._row_messages_src = row_to_message  # identity of the caller's object: callers that pass it every time do not re-upload
        self._row_messages = np.array(row_to_message, dtype=np.int64).reshape(-1)  # a snapshot: never an alias of the caller's array
        self._row_messages_rows = -1  # (re-)uploaded on the next message lookup

    def _check_row_messages(self) -> None:
        if self._row_messages is None:
            raise RuntimeError("set_row_messages() first")
        if len(self._row_messages) < self._count:
            raise ValueError(f"the row -> message map covers {len(self._row_messages)} rows, the index has {self._count}")

    def _messages_engine(self):
        """engine with corpus AND map synced, or None when the aggregation has to run on the host (device group)."""
        self._check_row_messages()
        eng = self._sync_device()
        if not isinstance(eng, _native.Engine):
            return None
        if self._row_messages_rows != self._count:
            eng.set_row_messages(self._row_messages[: self._count])
            self._row_messages_rows = self._count
        return eng

    def _messages_group(self, eng, max_messages: int):
        """The device group `eng` with the map's slices synced to its current bounds, when it serves top-messages lookups itself
        (`DeviceGroup.search_top_messages`: every engine real, option "top_messages" on, 1 <= max_messages <= 16384); else None."""
        if not (hasattr(eng, "top_messages_capable") and hasattr(eng, "search_top_messages") and 1 <= max_messages <= _native.MAX_LARGE_K
                and eng.top_messages_capable()):
            return None
        if self._row_messages_rows != self._count or getattr(eng, "row_messages_bounds", None) != tuple(eng.bounds):
            held = self._row_messages[: self._count]
            eng.set_row_messages(held, int(held.max()) + 1 if self._count else 0)
            self._row_messages_rows = self._count
        return eng

    def _host_rerank(self, hits, max_matches, accept=None) -> list[ScoredInt]:
        best: dict[int, float] = {}
        for h in hits:
            msg = int(self._row_messages[h.item])
            if msg < 0 or (accept is not None and msg not in accept):
                continue
            if msg not in best:
                best[msg] = h.score  # hits arrive best first: the first occurrence is the best score
        out = [ScoredInt(m, sc) for m, sc in best.items()]
        return out if max_matches is None else out[:max_matches]

    def lookup_messages_by_embedding(
        self,
        embedding: NormalizedEmbedding,
        max_matches: int | None = None,
        threshold_score: float | None = None,
        accept_ordinals=None,
    ) -> list[ScoredInt]:
        """`SqliteMessageTextIndex.lookup_by_embedding` / `lookup_in_subset_by_embedding`
        (storage/sqlite/messageindex.py:296-326, 182-257) as ONE device submission: full-corpus top-`max_matches` chunk
        rows (None -> 10, like `fuzzy_lookup_embedding`), THEN the membership filter on their message ordinals
        (`accept_ordinals`, the provider's `ordinals_set`), THEN best score per message, THEN the cut -- the provider's
        order, so the result is the provider's (possibly fewer than `max_matches` messages).  -> [ScoredInt(message, score)]."""
        max_hits, thr = self._limits(max_matches, threshold_score)
        if self._count == 0:
            return []
        eng = self._messages_engine()
        cut = max_hits if max_matches is not None else max(max_hits, 1)
        if eng is None or not (1 <= max_hits <= _PAGE):
            hits = self.fuzzy_lookup_embedding(embedding, max_hits=max_matches, min_score=threshold_score)
            return self._host_rerank(hits, max_matches, None if accept_ordinals is None else set(int(x) for x in accept_ordinals))
        acc = self._accept_array(None if accept_ordinals is None else np.fromiter((int(x) for x in accept_ordinals), dtype=np.int64))
        msgs, scs = eng.search_messages(embedding, max_hits, thr, cut, accept=acc)
        return [ScoredInt(int(m), float(sc)) for m, sc in zip(msgs.tolist(), scs.tolist())]

    def lookup_messages_in_subset_by_embedding(
        self,
        embedding: NormalizedEmbedding,
        rows_of_subset: list[int],
        max_matches: int | None = None,
        threshold_score: float | None = None,
    ) -> list[ScoredInt]:
        """The in-memory provider's form (storage/memory/messageindex.py:173-207 via knowpro/textlocindex.py:164-177): a
        true subset gather over the given index positions, then best score per message, sorted."""
        max_hits, thr = self._limits(max_matches, threshold_score)
        if len(rows_of_subset) == 0 or self._count == 0:
            return []
        eng = self._messages_engine()
        if eng is None or not (1 <= max_hits <= _PAGE):
            hits = self.fuzzy_lookup_embedding_in_subset(embedding, rows_of_subset, max_hits=max_matches, min_score=threshold_score)
            return self._host_rerank(hits, None)
        rows = self._wrap_subset(rows_of_subset, self._count)[1]
        msgs, scs = eng.search_messages(embedding, max_hits, thr, max_hits, subset_rows=rows)
        return [ScoredInt(int(m), float(sc)) for m, sc in zip(msgs.tolist(), scs.tolist())]

    # ------------------------------------------------------------------ scoped and batched message lookups (additive)
    def message_mask(self, message_ordinals) -> RowMask:
        """A scope of MESSAGE ordinals -> the `RowMask` of their chunk rows: equals
        row_mask(np.isin(row_messages[:len(self)], message_ordinals) & (row_messages[:len(self)] >= 0)) -- ordinals that name no message
        (negative, or beyond the map's largest) are ignored, rows without a message (-1) are never allowed.  Needs `set_row_messages`.  On a
        single-GPU engine only the ordinals travel: the mask is built from the device copy of the map (tavb_mask_from_messages) and
        expanded there, the scope never becomes a host row list.  Device groups and test doubles build the bool array on the host."""
        self._check_row_messages()
        acc = np.asarray(message_ordinals if isinstance(message_ordinals, np.ndarray) else list(message_ordinals))
        if acc.size and acc.dtype.kind not in "iu":
            raise TypeError("message ordinals must be integers")
        acc = acc.astype(np.int64, copy=False).reshape(-1)
        n = self._count
        if n == 0:
            return RowMask(self, 0, 0, flat=np.zeros(0, np.int64))
        eng = self._messages_engine()
        if eng is not None and self._masked_native(eng) and hasattr(eng, "mask_from_messages"):
            dev_rows, count, dev_bits = eng.mask_from_messages(self._accept_array(acc))
            return RowMask(self, n, count, dev_rows=dev_rows, dev_bits=dev_bits)
        held = self._row_messages[:n]
        return self.row_mask(np.isin(held, acc) & (held >= 0))

    def lookup_messages_by_embedding_masked(
        self,
        embedding: NormalizedEmbedding,
        allowed,
        max_matches: int | None = None,
        threshold_score: float | None = None,
    ) -> list[ScoredInt]:
        """`lookup_messages_in_subset_by_embedding` among the rows `allowed` names (a mask, see `row_mask`; a `RowMask`, e.g. from
        `message_mask`): equals lookup_messages_in_subset_by_embedding(embedding, np.flatnonzero(allowed).tolist(), max_matches,
        threshold_score)."""
        return self.lookup_messages_by_embeddings_masked(self._batch_of_one(embedding), allowed, max_matches, threshold_score)[0]

    def lookup_messages_by_embeddings_masked(
        self,
        embeddings: NormalizedEmbeddings,
        allowed,
        max_matches: int | None = None,
        threshold_score: float | None = None,
    ) -> list[list[ScoredInt]]:
        """Batch form over ONE mask: equals [lookup_messages_in_subset_by_embedding(e, np.flatnonzero(allowed).tolist(), max_matches,
        threshold_score) for e in embeddings] -- a scoped search (the best `max_matches` chunk rows AMONG the allowed ones, then best score
        per message), not the post-filter of `lookup_messages_by_embedding(accept_ordinals=...)`.  Rows of the mask that have no message
        are skipped by the aggregation.  `threshold_score` may be a sequence with one threshold per query.

        On a single-GPU engine with 1 <= max_matches <= 256 it is ONE submission (tavb_search_messages_masked): the masked batch on the
        route `fuzzy_lookup_embeddings_masked` would take (options "mask_tile" / "mask_wide"; `engine.get_option("masked_route")` tells
        which ran), the key lists left on the device, one launch of the message aggregation for all queries, one copy back.  On the row
        list (route 1) and on the wide filter tile (route 3) the result equals the sequential calls bit for bit -- messages, float32 scores
        and counts; on the 32/64-query tile (route 2) the messages are identical except among float32 near-ties and the scores agree
        within 1e-5.  Everything else (max_matches outside 1..256, device groups, test doubles) goes through
        `fuzzy_lookup_embeddings_masked` and the host aggregation."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_matches, threshold_score)
        self._check_row_messages()
        mask = self._resolve_mask(allowed)
        nq = len(queries)
        if self._count == 0 or mask.count == 0 or nq == 0:
            return [[] for _ in range(nq)]
        eng = self._messages_engine()
        if eng is not None and self._masked_native(eng) and hasattr(eng, "search_messages_masked") and mask.dev_rows is not None and 1 <= max_hits <= _PAGE:
            route = self._masked_route(eng, mask, nq, max_hits)
            msgs, scs, cnts = eng.search_messages_masked(queries, mask.dev_bits, mask.dev_rows, max_hits, thr, max_hits, route, span=mask.span)
            return _scored_lists(msgs, scs, cnts, max_hits)
        lists = self.fuzzy_lookup_embeddings_masked(queries, mask, max_matches, threshold_score if per_query is None else per_query)
        return [self._host_rerank(hits, None) for hits in lists]

    def lookup_messages_by_embeddings_scoped(
        self,
        embeddings: NormalizedEmbeddings,
        scopes,
        max_matches: int | None = None,
        threshold_score: float | None = None,
    ) -> list[list[ScoredInt]]:
        """`fuzzy_lookup_embeddings_scoped` aggregated to messages: one scope per query, and per query the result equals
        lookup_messages_by_embedding_masked(e, s, max_matches, threshold_score_i).  `threshold_score` may be a sequence with one threshold
        per query.  When every scope is the same handle this IS `lookup_messages_by_embeddings_masked`.  Otherwise a single-GPU engine with
        1 <= max_matches <= 256 whose scopes hold their packed mask on the device makes ONE submission (tavb_search_messages_scoped: the
        scoped batch, its key lists left on the device, one launch of the message aggregation, one copy back), bit for bit the per-query
        calls on the row list -- or, where `fuzzy_lookup_embeddings_scoped` would take the 32/64-query tile (option "scope_tile"),
        tavb_search_messages_scoped_tile with the tile's contract: the same messages except among float32 near-ties -- or, where it would take
        the 128/256-query filter tile (option "scope_wide"), tavb_search_messages_scoped_wide, bit for bit again; everything else (max_matches outside 1..256, device groups, test doubles, a handle without a device mask)
        loops over `lookup_messages_by_embedding_masked`."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_matches, threshold_score)
        self._check_row_messages()
        nq = len(queries)
        handles = self._resolve_scopes(scopes, nq)
        if nq and all(h is handles[0] for h in handles):
            return self.lookup_messages_by_embeddings_masked(queries, handles[0], max_matches, threshold_score if per_query is None else per_query)
        order = self._scoped_order(handles)
        if self._count == 0 or not order:
            return [[] for _ in range(nq)]
        eng = self._messages_engine()
        if eng is not None and self._scoped_native(eng, "search_messages_scoped", handles, order, max_hits):
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
            wide = self._scoped_wide(eng, "search_messages_scoped_wide", handles, order, max_hits)
            span = None if wide is not None else self._scoped_tile(eng, "search_messages_scoped_tile", handles, order, max_hits)
            if wide is not None:
                m, s, c = eng.search_messages_scoped_wide(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                          np.ascontiguousarray(t[order]), max_hits, span=wide)
            elif span is not None:
                m, s, c = eng.search_messages_scoped_tile(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                          np.ascontiguousarray(t[order]), max_hits, span=span)
            else:
                m, s, c = eng.search_messages_scoped(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                     np.ascontiguousarray(t[order]), max_hits)
            msgs, scs, cnts = np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32), np.zeros(nq, np.int32)
            msgs[order], scs[order], cnts[order] = m, s, c
            return _scored_lists(msgs, scs, cnts, max_hits)
        return [self.lookup_messages_by_embedding_masked(q, handles[i], max_matches, threshold_score if per_query is None else per_query[i])
                for i, q in enumerate(queries)]

    def lookup_messages_by_embeddings(
        self,
        embeddings: NormalizedEmbeddings,
        max_matches: int | None = None,
        threshold_score: float | None = None,
        accept_ordinals=None,
    ) -> list[list[ScoredInt]]:
        """Batch form of `lookup_messages_by_embedding`: equals [lookup_messages_by_embedding(e, max_matches, threshold_score,
        accept_ordinals) for e in embeddings], on a single-GPU engine with 1 <= max_matches <= 256 as ONE submission
        (tavb_search_messages_batch: the batch's full-corpus top-k, the accept filter, the aggregation of every query in one launch).  Bit
        for bit wherever the batch route is (the streaming kernels, the wide tile + rescoring); a batch the 32/64-query tile serves agrees
        the way `fuzzy_lookup_embeddings` does there.  `threshold_score` may be a sequence with one threshold per query."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_matches, threshold_score)
        nq = len(queries)
        if self._count == 0 or nq == 0:
            return [[] for _ in range(nq)]
        accept = None if accept_ordinals is None else [int(x) for x in accept_ordinals]
        eng = self._messages_engine()
        if eng is None or not hasattr(eng, "search_messages_batch") or not (1 <= max_hits <= _PAGE):
            return [self.lookup_messages_by_embedding(q, max_matches, threshold_score if per_query is None else per_query[i], accept) for i, q in enumerate(queries)]
        acc = self._accept_array(None if accept is None else np.asarray(accept, dtype=np.int64).reshape(-1))
        cut = max_hits if max_matches is not None else max(max_hits, 1)
        msgs, scs, cnts = eng.search_messages_batch(queries, max_hits, thr, cut, accept=acc)
        return _scored_lists(msgs, scs, cnts, max_hits)

    # ------------------------------------------------------------------ top-k distinct messages (additive)
    def _collapse_to_messages(self, hits, max_messages: int) -> list[ScoredInt]:
        """Row hits (every survivor of a lookup) -> the best `max_messages` MESSAGES (0: all of them): per message the best score of its
        rows, rows without a message (-1) dropped, sorted by (score descending, message ordinal ascending)."""
        if not hits:
            return []
        n = len(hits)
        rows = np.fromiter((h.item for h in hits), dtype=np.int64, count=n)
        scs = np.fromiter((h.score for h in hits), dtype=np.float64, count=n)
        msgs = self._row_messages[rows]
        keep = msgs >= 0
        msgs, scs = msgs[keep], scs[keep]
        order = np.lexsort((msgs, -scs))
        msgs, scs = msgs[order], scs[order]
        first = np.sort(np.unique(msgs, return_index=True)[1])  # a message's first entry in that order carries its best score
        if max_messages:
            first = first[:max_messages]
        return list(map(ScoredInt, msgs[first].tolist(), scs[first].tolist()))

    @staticmethod
    def _top_messages_native(eng, max_messages: int) -> bool:
        """A single-GPU engine with the call, its "top_messages" option on (the default) and 1 <= max_messages <= 16384; device groups,
        test doubles, the option at 0 and every other max_messages take the all-survivor lookup and the host collapse."""
        return (isinstance(eng, _native.Engine) and hasattr(eng, "search_top_messages") and 1 <= max_messages <= _native.MAX_LARGE_K
                and eng.get_option("top_messages") != 0)

    @staticmethod
    def _top_messages_tile(eng, mask, nq: int) -> bool:
        """Whether a top-messages batch that `_top_messages_native` serves takes the 32/64-query tile (Engine.search_top_messages_tile)
        instead of the row scan: the engine has the call, the mask (if any) holds its packed bits and its span, and the option
        "top_messages_tile" (0 = never, the default; 2 = wherever the tile serves the shape; 1 = where tavb_plan_top_messages_tile
        expects it to win) says so."""
        if not (hasattr(eng, "search_top_messages_tile") and hasattr(eng, "plan_top_messages_tile")):
            return False
        if mask is not None and (mask.dev_bits is None or mask.span is None):
            return False
        opts = (eng.top_messages_tile_options() if hasattr(eng, "top_messages_tile_options") else
                tuple(eng.get_option(n) for n in ("top_messages_tile", "top_messages_tile_min_batch", "mask_tile_min_bytes", "mask_tile_pct")))
        mode, min_batch, min_bytes, pct = opts
        if mode == 0:
            return False
        if mode == 2:  # (one allowed row in a span of one, no floors: yes exactly when the tile serves the width)
            return bool(eng.plan_top_messages_tile(64, eng.dim, eng.dtype, 1, 1, 0, 0, 0))
        if mask is None:
            return bool(eng.plan_top_messages_tile(nq, eng.dim, eng.dtype, eng.rows, eng.rows, min_batch, min_bytes, pct))
        return bool(eng.plan_top_messages_tile(nq, eng.dim, eng.dtype, mask.count, mask.span[1] + 1 - mask.span[0] // 256 * 256, min_batch, min_bytes, pct))

    def lookup_top_messages_by_embedding(
        self,
        embedding: NormalizedEmbedding,
        max_messages: int | None = None,
        threshold_score: float | None = None,
        allowed=None,
    ) -> list[ScoredInt]:
        """The best `max_messages` MESSAGES (None -> 10): see `lookup_top_messages_by_embeddings`, of which this is the one-query form."""
        return self.lookup_top_messages_by_embeddings(self._batch_of_one(embedding), max_messages, threshold_score, allowed)[0]

    def lookup_top_messages_by_embeddings(
        self,
        embeddings: NormalizedEmbeddings,
        max_messages: int | None = None,
        threshold_score: float | None = None,
        allowed=None,
    ) -> list[list[ScoredInt]]:
        """Top-k DISTINCT messages ("collapsing"), per query: of every row that is inside `allowed` (a mask, see `row_mask`, or a `RowMask`
        from `row_mask`, `message_mask`, `range_mask` or mask algebra; None: every row), has a message (`set_row_messages`, not -1) and
        scores >= `threshold_score` (NaN never passes), each message gets the best score of its rows; the `max_messages` (None -> 10)
        messages with the highest best score are returned, sorted by that score descending, ties by ascending message ordinal -- always
        min(max_messages, messages with a passing row) of them.  `lookup_messages_by_embedding` instead collapses the best `max_matches`
        chunk ROWS and may return far fewer messages.  Scores are `fuzzy_lookup_embedding`'s float32 scores bit for bit;
        `threshold_score` may be a sequence with one threshold per query.

        On a single-GPU engine with 1 <= max_messages <= 16384 (and a mask that holds its row list on the device) it is ONE submission
        (tavb_search_top_messages, engine option "top_messages", default 1): per eight queries one corpus pass that keeps one maximum per
        message on the device, then the exact device top-k over the messages.  On a device group (`devices=[...]`) under the same
        conditions every shard runs that call over its rows (or its part of the mask) and returns its own best `max_messages` messages
        with global message ordinals; the lists are merged on the host, one maximum per message and then the best `max_messages`
        (`DeviceGroup.search_top_messages`, tavb_merge_top_messages_host) -- the single-GPU answer, bit for bit where the shards' rows
        are a multiple of 16 bytes.  Everything else -- max_messages 0 (every message) or beyond 16384, test doubles, "top_messages" = 0
        -- takes the all-survivor lookup (`fuzzy_lookup_embedding(s)` / `_masked` at max_hits = 0) and collapses on the host, with the
        same result.  One scope per query in one submission is `lookup_top_messages_by_embeddings_scoped`.  Not served here:
        `FusedIndexQuery`.

        Engine option "top_messages_tile" (default 0) moves the native route onto the 32/64-query MFMA tile
        (tavb_search_top_messages_tile: one corpus pass per 64 queries instead of one per eight; rows of a multiple of 64 bytes; a mask
        must hold its packed bits): 1 = where tavb_plan_top_messages_tile expects it to win, 2 = wherever the tile serves the shape.
        Scores are then the tile's own -- within a few ulp of `fuzzy_lookup_embedding`'s, NOT bit for bit, as on every other route of that
        tile -- which is why the switch is off unless a deployment flips it."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_messages, threshold_score)
        self._check_row_messages()
        mask = None if allowed is None else self._resolve_mask(allowed)
        nq = len(queries)
        if self._count == 0 or nq == 0 or (mask is not None and mask.count == 0):
            return [[] for _ in range(nq)]
        eng = self._messages_engine()
        if eng is not None and self._top_messages_native(eng, max_hits) and self._top_messages_tile(eng, mask, nq):
            msgs, scs, cnts = eng.search_top_messages_tile(queries, max_hits, thr, dev_bits=None if mask is None else mask.dev_bits,
                                                           span=None if mask is None else mask.span)
            return _scored_lists(msgs, scs, cnts, max_hits)
        if eng is not None and self._top_messages_native(eng, max_hits) and (mask is None or (self._masked_native(eng) and mask.dev_rows is not None)):
            msgs, scs, cnts = eng.search_top_messages(queries, max_hits, thr, dev_rows=None if mask is None else mask.dev_rows)
            return _scored_lists(msgs, scs, cnts, max_hits)
        if eng is None and (mask is None or mask.shards is not None):
            group = self._sync_device()
            if (mask is None or self._masked_group(group)) and self._messages_group(group, max_hits) is not None:
                if mask is not None and mask.bounds != tuple(group.bounds):  # (as `fuzzy_lookup_embeddings_masked` cuts a handle again)
                    mask.shards, _, mask.bounds = group._rows_to_handles(mask.flat())
                msgs, scs, cnts = group.search_top_messages(queries, max_hits, thr, handles=None if mask is None else mask.shards)
                return _scored_lists(msgs, scs, cnts, max_hits)
        min_score = threshold_score if per_query is None else per_query
        lists = self.fuzzy_lookup_embeddings(queries, 0, min_score) if mask is None else self.fuzzy_lookup_embeddings_masked(queries, mask, 0, min_score)
        return [self._collapse_to_messages(hits, max_hits) for hits in lists]

    @classmethod
    def _top_messages_scoped_native(cls, eng, handles, order, max_messages: int) -> bool:
        """The one-call route of a scoped top-messages batch: `_top_messages_native` on an engine that has the scoped call, the option
        "top_messages_scoped" on (the default) and every searched scope holding its packed mask on the device."""
        return (eng is not None and hasattr(eng, "search_top_messages_scoped") and cls._top_messages_native(eng, max_messages)
                and eng.get_option("top_messages_scoped") != 0 and all(handles[i].dev_bits is not None for i in order))

    def lookup_top_messages_by_embeddings_scoped(
        self,
        embeddings: NormalizedEmbeddings,
        scopes,
        max_messages: int | None = None,
        threshold_score: float | None = None,
    ) -> list[list[ScoredInt]]:
        """`lookup_top_messages_by_embeddings` for queries that carry their OWN scopes -- the lookups of one compiled question, each under
        its `when` filter: `scopes` is a sequence with one entry per query, each anything `allowed` takes there (a `RowMask` of this index
        from `row_mask`, `message_mask`, `range_mask` or mask algebra, a bool array, a bool tensor).  Equals
        [lookup_top_messages_by_embedding(e, max_messages, threshold_score_i, s) for e, s in zip(embeddings, scopes)]: a message whose
        chunks lie in several queries' scopes gets, for each query, the best score among the rows of THAT query's scope.
        `threshold_score` may be a sequence with one threshold per query.  A different number of scopes and embeddings raises ValueError;
        a handle of another index, another length or from before an edit raises what the masked lookups raise.

        When every scope is the same handle this IS `lookup_top_messages_by_embeddings` over it.  Otherwise, on a single-GPU engine with
        1 <= max_messages <= 16384 whose scopes all hold their packed mask on the device (engine options "top_messages" and
        "top_messages_scoped", both default 1), the batch is ONE submission (tavb_search_top_messages_scoped): the queries are ordered so
        that identical handles sit next to each other and go in passes of eight over the UNION of the pass' scopes -- built, listed and
        tested on the device; a row several scopes share is read once per pass -- and the answers come back in the caller's order, bit
        for bit those of the per-query calls: message ordinals, float32 scores and counts.  A query whose scope is empty gets an empty
        answer and takes no slot.  `engine.get_option("masked_route")` is then 9.

        Everything else loops over `lookup_top_messages_by_embedding`: max_messages 0 or beyond 16384 (the host collapse), device groups
        (every iteration then takes the group's own top-messages route), test doubles, either option at 0, and a handle without a
        device mask.  Not served here: `FusedIndexQuery`,
        the MFMA tiles; queries are not reordered by how much their scopes overlap -- only identical handles are grouped."""
        queries, max_hits, thr, per_query = self._batch_args(embeddings, max_messages, threshold_score)
        self._check_row_messages()
        nq = len(queries)
        handles = self._resolve_scopes(scopes, nq)
        min_score = threshold_score if per_query is None else per_query
        if nq and all(h is handles[0] for h in handles):
            return self.lookup_top_messages_by_embeddings(queries, max_messages, min_score, allowed=handles[0])
        order = self._scoped_order(handles)
        if self._count == 0 or not order:
            return [[] for _ in range(nq)]
        eng = self._messages_engine()
        if self._top_messages_scoped_native(eng, handles, order, max_hits):
            t = np.broadcast_to(np.asarray(thr, dtype=np.float32), (nq,))
            m, s, c = eng.search_top_messages_scoped(np.ascontiguousarray(queries[order]), [handles[i].dev_bits for i in order], max_hits,
                                                     np.ascontiguousarray(t[order]))
            msgs, scs, cnts = np.zeros((nq, max_hits), np.int64), np.zeros((nq, max_hits), np.float32), np.zeros(nq, np.int32)
            msgs[order], scs[order], cnts[order] = m, s, c
            return _scored_lists(msgs, scs, cnts, max_hits)
        return [self.lookup_top_messages_by_embedding(q, max_messages, min_score if per_query is None else per_query[i], handles[i])
                for i, q in enumerate(queries)]

    async def fuzzy_lookup(
        self,
        key: str,
        max_hits: int | None = None,
        min_score: float | None = None,
        predicate: Callable[[int], bool] | None = None,
    ) -> list[ScoredInt]:
        if max_hits is None:
            max_hits = self.settings.max_matches
        if min_score is None:
            min_score = self.settings.min_score
        embedding = await self.get_embedding(key)
        return self.fuzzy_lookup_embedding(embedding, max_hits=max_hits, min_score=min_score, predicate=predicate)

    # ------------------------------------------------------------------ masks carried through row edits (additive)
    def _carried(self, carry) -> list[RowMask]:
        """`carry=` of an edit -> its handles, each once, refused as `_resolve_mask` refuses them -- before anything is edited."""
        out: list[RowMask] = []
        for h in (carry,) if isinstance(carry, RowMask) else tuple(carry):
            if not isinstance(h, RowMask):
                raise TypeError(f"carry takes RowMask handles of this index, got {type(h).__name__}")
            self._resolve_mask(h)
            if not any(h is x for x in out):
                out.append(h)
        return out

    def _carry_on_device(self, eng, handles) -> bool:
        """The device route of a carried edit: a single-GPU engine with tavb_mask_remap, and every handle holds its packed mask there."""
        return bool(handles) and self._masked_native(eng) and hasattr(eng, "mask_remap") and all(h.dev_bits is not None for h in handles)

    @staticmethod
    def _remap_on_device(eng, mode: int, dev_flags, old: int, new: int, handles, fill: bool) -> list[tuple]:
        """The handles' packed masks through one edit, 8 per call of tavb_mask_remap -> a quadruple (dev_rows, count, dev_bits, span) each.
        Nothing of the index or the handles is touched: the caller adopts the results once the edit itself is done."""
        most = _native.MAX_MASK_OPERANDS
        out: list[tuple] = []
        for i in range(0, len(handles), most):
            group = handles[i:i + most]
            out += eng.mask_remap(mode, dev_flags, old, new, [h.dev_bits for h in group], fill, counts=[h.count for h in group])
        return out

    def _fresh_mask(self, bools: np.ndarray) -> RowMask:
        """The host route's new handle: `row_mask`, or -- on an index that never reached a device -- the host list alone."""
        if self._engine is None:
            flat = np.flatnonzero(bools)
            return RowMask(self, len(bools), len(flat), flat=flat)
        return self.row_mask(bools)

    def _adopt_masks(self, handles, fresh) -> None:
        """Every handle takes over what its fresh twin -- a `RowMask`, or a quadruple of `_remap_on_device` -- holds, in place: the
        length, the count, the epoch, the lists, the packed mask and the span; its route plans are emptied with them."""
        for h, f in zip(handles, fresh):
            if not isinstance(f, RowMask):
                dev_rows, count, dev_bits, span = f
                f = RowMask(self, self._count, count, dev_rows=dev_rows, dev_bits=dev_bits, span=span)
            for slot in RowMask.__slots__:
                if slot != "_owner":
                    setattr(h, slot, getattr(f, slot))

    def extend_masks(self, *masks, new: bool = False) -> None:
        """Bring `RowMask` handles that were built at a smaller length -- before rows were appended by `add_embedding(s)` / `add_key(s)` --
        to len(self), IN PLACE: the rows they name stay, the appended rows are clear, or set with `new=True`; equals
        row_mask(np.concatenate([bools, np.full(len(self) - len(bools), new)])).  A handle already at the current length is left alone.
        Handles of another index, handles made before a removal or an insertion that was not handed them (`carry=`), and handles longer
        than the index raise ValueError, before any handle changes.  On a single-GPU engine handles that hold their packed mask on the
        device are extended there (tavb_mask_remap, 8 per call; only `new` and the two lengths travel); everything else goes through
        the host bool array and `row_mask`."""
        n = self._count
        todo: list[RowMask] = []
        for h in masks:
            if not isinstance(h, RowMask):
                raise TypeError(f"extend_masks takes RowMask handles of this index, got {type(h).__name__}")
            if h._owner() is not self:
                raise ValueError("this RowMask was built by another index")
            if h.epoch != self._removal_epoch:
                raise ValueError(f"this RowMask was built before rows were {self._epoch_change} the index: build it again")
            if h.rows > n:
                raise ValueError(f"mask covers {h.rows} rows, the index has {n}")
            if h.rows < n and not any(h is x for x in todo):
                todo.append(h)
        eng = self._engine
        for old in sorted({h.rows for h in todo}):
            group = [h for h in todo if h.rows == old]
            if self._carry_on_device(eng, group):
                fresh = self._remap_on_device(eng, _native.REMAP_APPEND, None, old, n, group, bool(new))
            else:
                fresh = []
                for h in group:
                    b = np.zeros(old, dtype=bool)
                    b[h.flat()] = True
                    fresh.append(self._fresh_mask(np.concatenate([b, np.full(n - old, bool(new))])))
            self._adopt_masks(group, fresh)

    # ------------------------------------------------------------------ removal (additive)
    def _removal_flags(self, which) -> tuple[np.ndarray | None, RowMask | None, int]:
        """What `remove_rows` was handed -> (bool [len(self)] of the rows to remove, or None when a RowMask's packed mask on the device says
        it; that RowMask; how many rows go)."""
        n = self._count
        if isinstance(which, RowMask):
            mask = self._resolve_mask(which)
            if mask.dev_bits is not None:
                return None, mask, mask.count
            return self._mask_bools(mask), None, mask.count
        a = np.asarray(which)
        if a.dtype == np.bool_:
            if a.ndim != 1 or a.shape[0] != n:
                raise ValueError("boolean array argument obj to delete must be one dimensional and match the axis length of " + str(n))
            return a, None, int(np.count_nonzero(a))
        if a.size == 0:
            return np.zeros(n, dtype=bool), None, 0
        if a.dtype.kind not in "iu":
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        a = a.reshape(-1).astype(np.int64)
        bad = a[(a < -n) | (a >= n)]
        if bad.size:
            raise IndexError(f"index {int(bad[0])} is out of bounds for axis 0 with size {n}")
        flags = np.zeros(n, dtype=bool)
        flags[a] = True  # (negatives wrap, duplicates fall together: np.delete's rules)
        return flags, None, int(np.count_nonzero(flags))

    def remove_rows(self, which, carry=()) -> int:
        """Remove rows -> how many went.  `which`: integer ordinals with np.delete's rules (duplicates allowed, negatives wrap, out of range
        raises IndexError), a bool array of length len(self), or a `RowMask` of this index.  Defined as the reference class with
        `_vectors = np.delete(_vectors, which, axis=0)`: later ordinals shift down -- the removal the reference leaves as a TODO
        (storage/sqlite/reltermsindex.py:181-192, knowpro/fuzzyindex.py:113-127).  On a single-GPU engine the device corpus is compacted on
        the device (tavb_compact_rows): a mirror is not uploaded again, a device-only corpus is not copied to the host, a RowMask's packed
        mask is used where it is; ordinals and bool arrays travel as rows / 8 bytes.  The host matrix, when there is one, is compacted in
        its growth buffer -- unless somebody else holds it (a matrix adopted by deserialize(), a view handed out by serialize()): then the
        index moves to a buffer of its own, as np.delete would.  The row -> message map loses the same rows.  Every `RowMask` built before
        the call raises ValueError from then on -- except the handles named in `carry`: they are updated IN PLACE and name the same
        vectors afterwards as before, minus the removed ones (row_mask(np.delete(bools, which)); a handle that is also `which` becomes the
        empty mask).  On a single-GPU engine carried handles that hold their packed mask on the device are remapped there, under the
        removal flags the compaction reads (tavb_mask_remap, 8 per call): nothing of them visits the host but their counts and spans.
        Everything else -- device groups, handles with a host list only -- goes through the host bool arrays and `row_mask`.  With no
        row to remove nothing changes and every handle stays as it is.  A device group (`devices=[...]`) removes on the host and
        uploads again."""
        carried = self._carried(carry)
        flags, mask, removed = self._removal_flags(which)
        if removed == 0:
            return 0
        n = self._count
        eng = self._engine
        native = eng is not None and hasattr(eng, "compact_rows")  # (a device group has no such call: the host route)
        if self._device_only is not None and not native:
            self._materialize_host()  # a device group: the host route
        if native and self._device_only is None:
            eng = self._sync_device()  # rows appended or edited since the last lookup reach the mirror first
        need_host_list = self._device_only is None or self._row_messages is not None
        on_device = native and self._carry_on_device(eng, carried)
        if flags is None and (need_host_list or not native or (carried and not on_device)):
            flags = self._mask_bools(mask)
        held = [] if on_device else [self._mask_bools(h) for h in carried]  # (read before the count changes)
        if native:
            dev_bits = mask.dev_bits if mask is not None else eng.mask_bits_to_device(_native.pack_mask_bits(flags))
            if on_device:  # (fresh tensors: neither the handles nor the flags change before the rows have moved)
                remapped = self._remap_on_device(eng, _native.REMAP_REMOVE, dev_bits, n, n - removed, carried, False)
            kept = eng.compact_rows(dev_bits)
            if kept != n - removed:
                raise RuntimeError(f"the device kept {kept} rows of {n}, expected {n - removed}")
        if self._device_only is not None:
            self._device_only = eng.corpus
            self._dev_rows, self._dev_valid = n - removed, True
        else:
            keep = ~flags
            first = int(np.argmax(flags))
            if self._handed_out or self._view_out:
                # the caller's own matrix, or one somebody holds a view of: np.delete leaves theirs as it is
                fresh = np.empty((max(n - removed, 4), self._embedding_size), dtype=np.float32)
                fresh[: n - removed] = self._host[:n][keep]
                self._host = fresh
                self._handed_out = self._view_out = False
                self._dev_fingerprint = None
            else:
                # in the growth buffer, a block at a time: a block's kept rows are copied out and land at or below where they were
                dst, block = first, max(1, (64 << 20) // max(self._host.shape[1] * 4, 1))
                row_bytes = self._host.strides[0]
                for b0 in range(first, n, block):
                    k = keep[b0 : b0 + block]
                    if k.all() and self._host.flags.c_contiguous:  # a whole block moves down: one pass (the ranges may overlap)
                        ctypes.memmove(self._host.ctypes.data + dst * row_bytes, self._host.ctypes.data + b0 * row_bytes, len(k) * row_bytes)
                        dst += len(k)
                        continue
                    part = self._host[b0 : b0 + len(k)][k]
                    self._host[dst : dst + len(part)] = part
                    dst += len(part)
            if native:
                self._dev_rows, self._dev_valid = n - removed, True
            else:
                self._dev_rows, self._dev_valid = 0, False
        self._count = n - removed
        if self._row_messages is not None:
            self._row_messages = np.delete(self._row_messages, np.flatnonzero(flags))
            self._row_messages_src = None  # (the caller's object describes the rows as they were)
            self._row_messages_rows = -1
        self._subset_cache = None
        self._removal_epoch += 1
        self._epoch_change = "removed from"
        if carried:
            self._adopt_masks(carried, remapped if on_device else [self._fresh_mask(b[~flags]) for b in held])
        return removed

    def remove_at(self, pos: int) -> None:
        """The method the reference keeps commented out (knowpro/fuzzyindex.py:113-127): remove the embedding at `pos`."""
        if not 0 <= pos < self._count:
            raise IndexError(f"Index {pos} out of bounds for embedding index of size {len(self)}")
        self.remove_rows([pos])

    # ------------------------------------------------------------------ insertion and overwrite (additive)
    def _rows_argument(self, embeddings) -> np.ndarray:
        """One row [dim] or rows [m, dim] -> float32 [m, dim] of this index' width (learned here on an empty index of unknown width)."""
        rows = np.asarray(embeddings, dtype=np.float32)
        if rows.ndim == 1:
            rows = rows.reshape(1, -1)
        if rows.ndim != 2:
            raise ValueError(f"Expected 1D or 2D embeddings array, got {rows.ndim}D")
        if self._embedding_size == 0 and rows.shape[1] > 0:
            self._set_embedding_size(rows.shape[1])
        if rows.shape[1] != self._embedding_size:
            raise ValueError(f"Embedding size mismatch: expected {self._embedding_size}, got {rows.shape[1]}")
        return rows

    @staticmethod
    def _insert_positions(at, n: int, m: int) -> np.ndarray:
        """np.insert's rule: where the m new rows stand in the matrix of n + m rows (int64 [m], row j of the values at [j])."""
        a = np.asarray(at)
        if a.dtype.kind not in "iu" and a.size:
            raise IndexError("arrays used as indices must be of integer (or boolean) type")
        if a.ndim > 1:
            raise ValueError("index array argument obj to insert must be one dimensional or scalar")
        idx = a.reshape(-1).astype(np.int64)
        bad = idx[(idx < -n) | (idx > n)]
        if bad.size:
            raise IndexError(f"index {int(bad[0])} is out of bounds for axis 0 with size {n}")
        idx[idx < 0] += n
        if idx.size == 1:  # one position: every row goes in front of it, in order
            return idx[0] + np.arange(m, dtype=np.int64)
        if idx.size != m:
            raise ValueError(f"shape mismatch: {m} rows cannot be inserted at {idx.size} positions")
        order = np.lexsort((idx,))  # (a stable sort: equal positions keep their order)
        idx[order] += np.arange(m, dtype=np.int64)
        return idx

    def insert_rows(self, at, embeddings, row_messages=None, carry=(), carry_new: bool = False) -> int:
        """Insert rows -> how many went in.  Defined as the reference class with `_vectors = np.insert(_vectors, at, embeddings, axis=0)`:
        `embeddings` is one row [dim] or [m, dim]; `at` one integer (all m rows go in front of old row `at`; `at == len(self)` appends) or
        a sequence of m integers (row j goes in front of old row at[j]; equal positions keep their order; one row and many positions
        inserts the row at each); negatives wrap, anything outside [-n, n] or a non-integer `at` raises IndexError, a width mismatch
        ValueError.  Later ordinals shift up -- the insertion the reference keeps commented out (knowpro/fuzzyindex.py:50-83).  On a
        single-GPU engine the device corpus is expanded on the device (tavb_expand_rows) and only the new rows travel
        (tavb_scatter_rows): a mirror is not uploaded again, a device-only corpus is not copied to the host.  The host matrix, when there
        is one, is opened up in its growth buffer, from the tail -- unless somebody else holds it (a matrix adopted by deserialize(), a
        view handed out by serialize()): then the index moves to a buffer of its own, as np.insert would.  The row -> message map gets
        `row_messages` (one int, or one per new row) at the same positions, -1 where none is given.  Every `RowMask` built before the
        call raises ValueError from then on -- except the handles named in `carry`: they are updated IN PLACE, keep the vectors they
        named and get `carry_new` (clear by default) at the new rows: row_mask(np.insert(bools, at, carry_new)) under the position rule
        of the rows.  On a single-GPU engine carried handles that hold their packed mask on the device are remapped there, under the
        hole flags the expansion reads (tavb_mask_remap, 8 per call); everything else goes through the host bool arrays and `row_mask`.
        A device group (`devices=[...]`) inserts on the host and uploads from the first new row."""
        carried = self._carried(carry)
        n = self._count
        new = self._rows_argument(embeddings)
        a = np.asarray(at)
        if new.shape[0] == 1 and a.ndim == 1 and a.size > 1:
            new = np.repeat(new, a.size, axis=0)
        m = new.shape[0]
        pos = self._insert_positions(a, n, m)
        msgs = None
        if row_messages is not None:
            msgs = np.asarray(row_messages, dtype=np.int64).reshape(-1)
            if msgs.size == 1:
                msgs = np.repeat(msgs, m)
            if msgs.size != m:
                raise ValueError(f"{msgs.size} row messages for {m} rows")
        if m == 0:
            return 0
        flags = np.zeros(n + m, dtype=bool)  # the holes, in the new index space
        flags[pos] = True
        first = int(pos.min())
        eng = self._engine
        native = eng is not None and hasattr(eng, "expand_rows") and hasattr(eng, "scatter_rows")  # (a device group has neither: the host route)
        on_device = native and n > 0 and self._carry_on_device(eng, carried)
        held = [] if on_device else [self._mask_bools(h) for h in carried]  # (read before the count changes)
        if n == 0:
            ordered = np.empty_like(new)
            ordered[pos] = new  # into an empty index: an append, in np.insert's order
            self.add_embeddings(None, ordered)
        else:
            if self._device_only is not None and not native:
                self._materialize_host()
            if native and self._device_only is None:
                eng = self._sync_device()  # rows appended or edited since the last lookup reach the mirror first
            if self._device_only is None:
                self._open_host_rows(flags, pos, new)
            if native:
                dev_flags = eng.mask_bits_to_device(_native.pack_mask_bits(flags))
                if on_device:  # (fresh tensors: the handles do not change before the rows have moved)
                    remapped = self._remap_on_device(eng, _native.REMAP_INSERT, dev_flags, n, n + m, carried, bool(carry_new))
                eng.expand_rows(dev_flags, n + m)
                eng.scatter_rows(new, pos.astype(np.int32))
                if self._device_only is not None:
                    self._device_only = eng.corpus
                self._dev_rows, self._dev_valid = n + m, True
            else:
                self._dev_rows = min(self._dev_rows, first)  # the upload does the rest
            self._count = n + m
        if self._row_messages is not None or msgs is not None:
            old = np.full(n, -1, dtype=np.int64)
            if self._row_messages is not None:
                k = min(n, len(self._row_messages))
                old[:k] = self._row_messages[:k]
            merged = np.empty(n + m, dtype=np.int64)
            merged[~flags] = old
            merged[pos] = -1 if msgs is None else msgs
            self._row_messages = merged
            self._row_messages_src = None  # (the caller's object describes the rows as they were)
            self._row_messages_rows = -1
        self._subset_cache = None
        self._removal_epoch += 1
        self._epoch_change = "inserted into"
        if carried and on_device:
            self._adopt_masks(carried, remapped)
        elif carried:
            fresh = []
            for b in held:
                grown = np.empty(n + m, dtype=bool)
                grown[~flags] = b
                grown[pos] = bool(carry_new)
                fresh.append(self._fresh_mask(grown))
            self._adopt_masks(carried, fresh)
        return m

    _host_block_bytes = 64 << 20  # the host matrix is opened up in blocks of about this size

    def _open_host_rows(self, flags: np.ndarray, pos: np.ndarray, new: np.ndarray) -> None:
        """The host side of `insert_rows`: the old rows move to the rows of `flags` that are clear, `new` goes to `pos`."""
        n, total = self._count, len(flags)
        if self._handed_out or self._view_out:
            # the caller's own matrix, or one somebody holds a view of: np.insert leaves theirs as it is
            fresh = np.empty((max(total, 4), self._embedding_size), dtype=np.float32)
            fresh[:total][~flags] = self._host[:n]
            self._host = fresh
            self._handed_out = self._view_out = False
            self._dev_fingerprint = None
        else:
            # in the growth buffer, a block at a time FROM THE TAIL: a block's old rows lie at or below it, and are copied out before the
            # block is written; the blocks still to come read only rows below them
            self._reserve(total - n)
            host = self._host
            first = int(pos.min())
            before = np.concatenate(([0], np.cumsum(flags, dtype=np.int64)))  # holes below a row
            block = max(1, self._host_block_bytes // max(host.shape[1] * 4, 1))
            row_bytes = host.strides[0]
            for b0 in reversed(range(first, total, block)):
                b1 = min(b0 + block, total)
                o0, o1 = b0 - int(before[b0]), b1 - int(before[b1])
                if o1 - o0 == b1 - b0 and host.flags.c_contiguous:  # no hole in the block: it moves up in one pass (the ranges may overlap)
                    if o0 != b0:
                        ctypes.memmove(host.ctypes.data + b0 * row_bytes, host.ctypes.data + o0 * row_bytes, (b1 - b0) * row_bytes)
                    continue
                part = host[o0:o1].copy()
                host[b0:b1][~flags[b0:b1]] = part
        self._host[pos] = new

    def insert_at(self, index: int, embeddings) -> None:
        """The method the reference keeps commented out (knowpro/fuzzyindex.py:50-83): insert one embedding, or a list of embeddings, in
        front of the row at `index`."""
        if not 0 <= index <= self._count:
            raise IndexError(f"Index {index} out of bounds for insertion in embedding index of size {len(self)}")
        rows = np.vstack([np.asarray(e, dtype=np.float32).reshape(1, -1) for e in embeddings]) if isinstance(embeddings, list) else embeddings
        self.insert_rows(int(index), rows)

    def set_rows(self, which, embeddings) -> int:
        """Overwrite rows -> how many rows were written.  Defined as `_vectors[which] = embeddings`: `which` is integer ordinals (negatives
        wrap, out of range raises IndexError, duplicates allowed: the last one wins), a bool array of length len(self), or a `RowMask`
        of this index (its rows in ascending order take `embeddings` in order); `embeddings` is [len(which), dim], or one row [dim]
        written to every named row.  The length does not change, `RowMask`s stay valid, the subset cache is kept.  On a single-GPU
        engine only the new rows travel (tavb_scatter_rows): a device-only corpus is not copied to the host, a mirror is not uploaded
        again, and the fp16 shadow and the row-norm maxima are brought up to date instead of being rebuilt; a host matrix is written
        as well.  A device group writes the host matrix and uploads from the first written row."""
        n = self._count
        if isinstance(which, RowMask):
            rows = self._resolve_mask(which).flat().astype(np.int64)
        else:
            a = np.asarray(which)
            if a.dtype == np.bool_:
                if a.ndim != 1 or a.shape[0] != n:
                    raise IndexError(f"boolean index did not match indexed array along axis 0; size of axis is {n} but size of corresponding boolean axis is {a.shape[0] if a.ndim else 1}")
                rows = np.flatnonzero(a).astype(np.int64)
            elif a.size == 0:
                rows = np.zeros(0, dtype=np.int64)
            elif a.dtype.kind not in "iu":
                raise IndexError("arrays used as indices must be of integer (or boolean) type")
            else:
                rows = a.reshape(-1).astype(np.int64)
                bad = rows[(rows < -n) | (rows >= n)]
                if bad.size:
                    raise IndexError(f"index {int(bad[0])} is out of bounds for axis 0 with size {n}")
                rows[rows < 0] += n
        if len(rows) == 0:
            return 0
        new = self._rows_argument(embeddings)
        if new.shape[0] == 1 and len(rows) != 1:
            new = np.repeat(new, len(rows), axis=0)
        if new.shape[0] != len(rows):
            raise ValueError(f"shape mismatch: {new.shape[0]} rows cannot be written to {len(rows)} positions")
        # duplicates are resolved here, the last one wins: the device never sees two writers of one row
        uniq, last = np.unique(rows[::-1], return_index=True)
        if len(uniq) != len(rows):
            new = new[len(rows) - 1 - last]
            rows = uniq
        eng = self._engine
        native = eng is not None and hasattr(eng, "scatter_rows")
        if self._device_only is not None and not native:
            self._materialize_host()
        if self._device_only is not None:
            eng.scatter_rows(new, rows.astype(np.int32))
            self._device_only = eng.corpus
            return len(rows)
        if native:
            eng = self._sync_device()  # the mirror as the matrix was: what was appended or edited before this call
        self._host[rows] = new
        if native:
            eng.scatter_rows(new, rows.astype(np.int32))
            if self._handed_out or self._view_out:
                self._dev_fingerprint = self._fingerprint()
        else:
            self._dev_rows = min(self._dev_rows, int(rows.min()))  # the upload does the rest
        return len(rows)

    # ------------------------------------------------------------------ bookkeeping
    def _set_embedding_size(self, size: int) -> None:
        assert size > 0
        self._embedding_size = size

    def clear(self) -> None:
        self._device_only = None
        self._subset_cache = None
        self._handed_out = False
        self._count = 0
        self._dev_rows = 0
        self._dev_valid = False
        if self._embedding_size > 0:
            self._host = np.zeros((0, self._embedding_size), dtype=np.float32)
        else:
            self._host = np.array([], dtype=np.float32)

    def get_embedding_at(self, pos: int) -> NormalizedEmbedding:
        if 0 <= pos < self._count:
            return self._vectors[pos]
        raise IndexError(f"Index {pos} out of bounds for embedding index of size {len(self)}")

    def serialize_embedding_at(self, pos: int) -> NormalizedEmbedding | None:
        return self._vectors[pos] if 0 <= pos < self._count else None

    def serialize(self) -> NormalizedEmbeddings:
        vectors = self._vectors
        if self._embedding_size > 0:
            assert vectors.shape == (len(vectors), self._embedding_size)
        return vectors  # the live matrix, like the reference (:271)

    def deserialize(self, data: NormalizedEmbeddings | None) -> None:
        if data is None:
            self.clear()
            return
        if self._embedding_size == 0:
            if data.ndim < 2 or data.shape[0] == 0:
                self.clear()  # nothing to learn the width from
                return
            self._set_embedding_size(data.shape[1])
        assert data.shape == (len(data), self._embedding_size), [data.shape, self._embedding_size]
        self._adopt_host(data)  # kept by reference, like the reference (:287)
