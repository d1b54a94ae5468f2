"""One VectorBase over several GPUs of a node, driven from ONE process and ONE thread.

typeagent is a single asyncio process whose query pipeline calls `fuzzy_lookup_embedding*` synchronously
(knowpro/query.py:886-934 of the reference), so the row-sharded corpus has to sit under one Python object: the SPMD
form (`sharded.py`, one process per GPU + RCCL) needs every rank to call collectively and is for the bench / servers.

`DeviceGroup` looks like `_native.Engine` to `VectorBase` (same methods), and holds one libtavb context + stream per
device.  Rows are sharded contiguously: shard g = rows [g*B, (g+1)*B), the last shard takes the appends (rebalanced
when it reaches twice the block size).  A lookup copies the query to every device and enqueues the per-shard scans back
to back (`tavb_search_begin`: nothing blocks), then collects the per-shard key lists (`tavb_search_end`), merges them
on the host (`tavb_merge_keys_host`: G x k keys per query -- cheaper than any collective) and
decodes.  Keys carry global ordinals and order by (score desc, ordinal asc), so the merged answer is the whole-corpus
answer, ties included.

max_hits 257 .. 16384 (`search_topk`, `search_subset_topk`): the exact device top-k of every shard (`tavb_search_topk_device`, enqueued
on all shards before anything is waited for) into one reused pinned buffer, merged on the host by `tavb_merge_topk_host`.

Masked lookups (`mask_to_rows`, `search_masked`): the mask is cut at the shard bounds, every slice is expanded on its shard's device
(`tavb_mask_expand`) into shard-local rows that stay there, and a batch of queries is ONE `tavb_search_subset_batch_device` per shard --
keys carrying global ordinals into the same pinned buffer, enqueued everywhere before anything is waited for -- merged on the host.

Top-k distinct messages (`set_row_messages`, `search_top_messages`): every shard holds its slice of the row -> message map with the global
message count, a batch is ONE `tavb_search_top_messages_device` per shard -- the shard's own best k messages, keys carrying global message
ordinals -- and the lists are merged on the host by `tavb_merge_top_messages_host`: one maximum per message, then the best k.
"""

from __future__ import annotations

import functools
import threading

import numpy as np

from . import _native


def _locked(method):
    """Hold the group's lock for the whole call: a lookup is `search_begin` on every device followed by `search_end` on every device, and
    each engine only locks per call -- two threads interleaving those pairs would collect each other's results (or trip the
    'tavb_search_end does not match the pending tavb_search_begin' check)."""

    @functools.wraps(method)
    def wrapper(self, *args, **kwargs):
        with self._lock:
            return method(self, *args, **kwargs)

    return wrapper


class DeviceGroup:
    def __init__(self, devices: list[int]):
        if len(devices) < 1:
            raise ValueError("devices must name at least one GPU")
        self.devices = [int(d) for d in devices]
        self.engines = [_native.Engine(d) for d in self.devices]
        self._lock = threading.RLock()
        self.block = 0  # rows per shard (the last shard may hold more)
        self.bounds = [0] * (len(self.devices) + 1)  # shard g = rows [bounds[g], bounds[g+1])
        self.rows = 0
        self.dim = 0
        self.dtype = _native.TAVB_F32
        self.ordinal_base = 0
        self.corpus = None  # truthy once rows are resident (VectorBase only tests it against None)
        self._topk_out: dict = {}  # (shards, nq, k) -> pinned int64 [shards, nq, k]: where the shards' large-k lists land
        self._topk_q: dict = {}  # ("pinned" or shard, nq, dim) -> the pinned staging buffer / that device's copy of the queries

    # -- lifecycle / options -------------------------------------------------------------------------------------
    def close(self) -> None:
        for e in self.engines:
            e.close()

    def set_option(self, name: str, value: int) -> None:
        for e in self.engines:
            e.set_option(name, value)

    def get_option(self, name: str) -> int:
        vals = [e.get_option(name) for e, lo, hi in self._active()] or [self.engines[0].get_option(name)]
        return max(vals) if name in ("last_flagged",) else vals[0]

    def profile_enable(self, on: bool = True) -> None:
        for e in self.engines:
            e.profile_enable(on)

    def profile_reset(self) -> None:
        for e in self.engines:
            e.profile_reset()

    def profile_read(self, kernel_id: int) -> tuple[float, int]:
        """(max over devices of the summed kernel time, launches on the first active device)"""
        parts = [e.profile_read(kernel_id) for e, lo, hi in self._active()] or [(0.0, 0)]
        return max(p[0] for p in parts), parts[0][1]

    def synchronize(self) -> None:
        for e in self.engines:
            e.synchronize()

    def _active(self):
        return [(e, self.bounds[g], self.bounds[g + 1]) for g, e in enumerate(self.engines) if self.bounds[g + 1] > self.bounds[g]]

    # -- corpus --------------------------------------------------------------------------------------------------
    def _layout(self, n: int, block: int) -> list[int]:
        g = len(self.engines)
        b = [min(i * block, n) for i in range(g)] + [n]
        return b

    @_locked
    def upload_rows(self, host_rows: np.ndarray, start: int, dtype: int, capacity_hint: int = 0) -> bool:
        """Make rows [start, start + len) of the sharded device copy equal `host_rows`.  Returns False (nothing done) when
        the shard layout has to change and the caller must upload from row 0 instead."""
        g = len(self.engines)
        n_new = start + host_rows.shape[0]
        dim = host_rows.shape[1]
        fresh = start == 0 or self.corpus is None or dim != self.dim or dtype != self.dtype
        if fresh and start != 0:
            return False
        if fresh:
            # balanced: ceil(n / g) rows per shard, every device reserving twice that; appends go to the last shard until it outgrows its
            # reservation, then the layout is rebuilt balanced.  (Round 3 doubled the BLOCK at a re-shard to re-shard less often: right after
            # one, 5 of 8 devices held rows and lookups ran ~1.8x slower until the index had doubled -- round-3 advice.  Balanced layouts
            # re-shard every time the index grows by 1/g: O(g) uploads per appended row when an index is grown row by row, 1 when it is
            # built in bulk; lookups always run on g equal shards.)
            self.block = max(1, -(-max(n_new, 1) // g))
        elif n_new > (g + 1) * self.block:  # the last shard would exceed twice the block: rebalance
            return False
        bounds = self._layout(n_new, self.block)
        for gi, e in enumerate(self.engines):
            lo, hi = bounds[gi], bounds[gi + 1]
            if hi <= lo:
                if e.rows:
                    e.clear()
                continue
            a = max(lo, start)
            if a >= hi and not fresh and e.rows == hi - lo:
                continue  # untouched shard
            e.ordinal_base = lo
            local = host_rows[a - start : hi - start] if a < hi else host_rows[:0]
            cap = 2 * self.block
            e.upload_rows(local, a - lo, dtype, capacity_hint=cap if (fresh or e.corpus is None) else 0)
        self.bounds, self.rows, self.dim, self.dtype = bounds, n_new, dim, dtype
        self.corpus = True
        return True

    @_locked
    def set_shard_tensors(self, tensors, ordinal_base: int = 0) -> None:
        """Adopt one device tensor per GPU (row shards in order) without a host copy."""
        if len(tensors) != len(self.engines):
            raise ValueError("one tensor per device")
        lo = 0
        bounds = [0]
        for e, t in zip(self.engines, tensors):
            e.set_corpus_tensor(t, ordinal_base=ordinal_base + lo)
            lo += int(t.shape[0])
            bounds.append(lo)
        self.bounds, self.rows = bounds, lo
        self.dim, self.dtype = self.engines[0].dim, self.engines[0].dtype
        self.block = max(1, max(b - a for a, b in zip(bounds, bounds[1:])))
        self.ordinal_base = ordinal_base
        self.corpus = list(tensors)

    @_locked
    def clear(self) -> None:
        for e in self.engines:
            e.clear()
        self.rows = 0
        self.bounds = [0] * (len(self.engines) + 1)

    # -- lookups -------------------------------------------------------------------------------------------------
    def _query(self, q) -> np.ndarray:
        a = np.ascontiguousarray(q, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] != self.dim:
            raise ValueError(f"shapes ({self.rows},{self.dim}) and {tuple(np.shape(q))} not aligned: query must have {self.dim} elements")
        return a

    @_locked
    def _gather(self, queries: np.ndarray, k: int, thrs: np.ndarray) -> np.ndarray:
        """-> merged uint64 [nq, k] keys over all shards"""
        act = self._active()
        nq = queries.shape[0]
        if not act:
            return np.zeros((nq, k), dtype=np.uint64)
        for e, lo, hi in act:  # enqueue everywhere first: the devices scan concurrently
            e.search_begin(queries, k, thrs)
        keys = np.empty((len(act), nq, k), dtype=np.uint64)
        for i, (e, lo, hi) in enumerate(act):
            e.search_end(nq, k, keys[i])
        return keys[0] if len(act) == 1 else _native.merge_keys(keys)

    def search(self, q, k: int, thr: np.float32):
        a = self._query(q)[None, :]
        ords, scs, cnts = _native.decode_keys(self._gather(a, k, np.asarray([thr], dtype=np.float32)))
        m = int(cnts[0])
        return ords[0, :m], scs[0, :m]

    def search_batch(self, queries, k: int, thrs):
        a = _native.batch_queries(queries, self.dim)
        return _native.decode_keys(self._gather(a, k, _native.batch_thresholds(thrs, a.shape[0])))

    # -- exact top-k past the fused selection (tavb_search_topk_device per shard + tavb_merge_topk_host) -------------------------
    def large_k_capable(self) -> bool:
        """Every engine is a real `_native.Engine` (has the device-resident large-k call) with the "large_k" option on."""
        return all(hasattr(e, "search_topk_device") and e.get_option("large_k") != 0 for e in self.engines)

    def _topk_lists(self, shards: int, nq: int, k: int):
        import torch

        key = (shards, nq, k)
        buf = self._topk_out.get(key)
        if buf is None:
            if len(self._topk_out) >= 8:
                self._topk_out.clear()
            buf = self._topk_out[key] = torch.empty(key, dtype=torch.int64).pin_memory()
        return buf

    def _device_queries(self, shards, a: np.ndarray):
        """The queries on every shard's device: `a` goes into ONE reused pinned buffer, the copies to the devices are enqueued back to back
        on torch's streams and each device is waited for once -- the engines run on streams of their own, so the rows must be there
        before their scans are enqueued.  shards: [(slot, engine)] -> one device tensor per shard."""
        import torch

        key = ("pinned",) + a.shape
        pinned = self._topk_q.get(key)
        if pinned is None:
            if len(self._topk_q) >= 32:
                self._topk_q.clear()
            pinned = self._topk_q[key] = torch.empty(a.shape, dtype=torch.float32).pin_memory()
        pinned.numpy()[...] = a
        out = []
        for g, e in shards:
            dq = self._topk_q.get((g,) + a.shape)
            if dq is None or dq.device.index != e.device:
                dq = self._topk_q[(g,) + a.shape] = torch.empty(a.shape, dtype=torch.float32, device=torch.device("cuda", e.device))
            dq.copy_(pinned, non_blocking=True)
            out.append(dq)
        for d in {e.device for g, e in shards}:
            torch.cuda.current_stream(d).synchronize()
        return out

    def _on_all_parts(self, parts, a: np.ndarray, k: int, enqueue) -> np.ndarray:
        """One device-resident lookup per part -- parts: [(slot, engine, ...)]; `enqueue(part, that device's copy of the queries `a`, that
        part's int64 [nq, k] of the pinned lists)` -- enqueued on every part before any is waited for -> the lists, uint64 [parts, nq, k]
        (a view of the reused pinned buffer)."""
        lists = self._topk_lists(len(parts), a.shape[0], k)
        dqs = self._device_queries([part[:2] for part in parts], a)
        for part, dq, out in zip(parts, dqs, lists):  # enqueue everywhere first: the devices scan concurrently
            enqueue(part, dq, out)
        for part in parts:
            part[1].synchronize()
        return lists.numpy().view(np.uint64)

    @_locked
    def search_topk(self, queries, k: int, thrs):
        """`Engine.search_topk` over the shards: queries f32 [nq, dim]; thrs float32 [nq] (or one for all); 1 <= k <= MAX_LARGE_K ->
        (ordinals [nq,k], scores [nq,k], counts [nq])."""
        a = _native.batch_queries(queries, self.dim)
        nq = a.shape[0]
        t = _native.batch_thresholds(thrs, nq)
        parts = [(g, e) for g, (e, lo, hi) in enumerate(self._active())]
        if not parts or nq == 0:
            return np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        keys = self._on_all_parts(parts, a, k, lambda part, dq, out: part[1].search_topk_device(dq, k, t, out_keys=out))
        return _native.decode_keys(keys[0] if len(parts) == 1 else _native.merge_topk_keys(keys))

    @_locked
    def search_subset_topk(self, q, rows: np.ndarray, k: int, thr: np.float32):
        """`Engine.search_subset_topk` over the shards: rows: int64 global corpus row per subset position -> (positions int64[m], scores
        float32[m]), ordered (score desc, position asc) like one device's."""
        import torch

        a = self._query(q)[None, :]
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        parts = []
        for g, (e, lo, hi) in enumerate(self._active()):
            idx = np.flatnonzero((rows >= lo) & (rows < hi))  # ascending positions: the remapped lists stay sorted among equal scores
            if idx.size:
                parts.append((g, e, idx, torch.from_numpy((rows[idx] - lo).astype(np.int32)).to(torch.device("cuda", e.device))))
        if not parts:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        keys = self._on_all_parts(parts, a, k, lambda part, dq, out: part[1].search_topk_device(dq, k, thr, out_keys=out, dev_rows=part[3])).copy()
        low = np.uint64(0xFFFFFFFF)
        for i, (g, e, idx, dev_rows) in enumerate(parts):  # positions in the shard's part of the subset -> positions in the caller's list
            row = keys[i, 0]
            live = row != 0
            local = (low - (row[live] & low)).astype(np.int64)
            row[live] = (row[live] & ~low) | (low - idx[local].astype(np.uint64))
        ords, scs, cnts = _native.decode_keys(keys[0] if len(parts) == 1 else _native.merge_topk_keys(keys))
        m = int(cnts[0])
        return ords[0, :m], scs[0, :m]

    # -- masked lookups (tavb_mask_expand + tavb_search_subset_batch_device per shard, merged on the host) ------------------------------
    def masked_capable(self) -> bool:
        """Every engine expands masks and searches their row list without waiting (`_native.Engine`); test doubles lack the methods."""
        return all(hasattr(e, "mask_to_rows") and hasattr(e, "search_subset_batch_device") for e in self.engines)

    @_locked
    def mask_to_rows(self, mask):
        """An allow-mask over the whole index -- a numpy bool array [rows] or a torch bool tensor [rows] on any device -- cut at the
        current `bounds` and expanded shard by shard on the shard's own device -> (handles: one per engine, torch int32 shard-local rows
        in ascending order, None where the shard has no allowed row; the total count; the bounds the mask was cut by)."""
        is_tensor = hasattr(mask, "is_cuda") and hasattr(mask, "dtype")
        handles, total = [None] * len(self.engines), 0
        for g, e in enumerate(self.engines):
            lo, hi = self.bounds[g], self.bounds[g + 1]
            if hi <= lo:
                continue
            part = mask[lo:hi]  # (one byte per row in either form: every cut is on a byte boundary, the shard packs its own bits)
            if is_tensor:
                import torch

                part = part.to(torch.device("cuda", e.device)).contiguous()
            dev_rows, count = e.mask_to_rows(part)
            if count:
                handles[g] = dev_rows
                total += int(count)
        return handles, total, tuple(self.bounds)

    @_locked
    def _rows_to_handles(self, flat: np.ndarray):
        """Ascending global rows (np.flatnonzero of a mask) -> what `mask_to_rows` returns for that mask under the current `bounds`."""
        flat = np.ascontiguousarray(flat, dtype=np.int64)
        cuts = np.searchsorted(flat, np.asarray(self.bounds, dtype=np.int64))
        handles = [None] * len(self.engines)
        for g, e in enumerate(self.engines):
            if cuts[g + 1] > cuts[g]:
                handles[g] = e.rows_to_device(flat[cuts[g] : cuts[g + 1]] - self.bounds[g])
        return handles, int(len(flat)), tuple(self.bounds)

    @_locked
    def search_masked(self, queries, handles, k: int, thrs):
        """`search_topk` among the rows of a mask (handles: `mask_to_rows` under the current bounds): queries f32 [nq, dim]; thrs float32
        [nq] (or one for all); 1 <= k <= MAX_LARGE_K -> (ordinals [nq,k], scores [nq,k], counts [nq]).  One batched call per shard that
        has a handle, all of them enqueued before any is waited for; shards without allowed rows are not visited."""
        a = _native.batch_queries(queries, self.dim)
        if len(handles) != len(self.engines):
            raise ValueError("one handle (or None) per device")
        nq = a.shape[0]
        t = _native.batch_thresholds(thrs, nq)
        parts = [(g, e, handles[g]) for g, e in enumerate(self.engines) if handles[g] is not None and self.bounds[g + 1] > self.bounds[g]]
        if not parts or nq == 0:
            return np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        keys = self._on_all_parts(parts, a, k, lambda part, dq, out: part[1].search_subset_batch_device(dq, part[2], k, t, out_keys=out, remap=True))
        if len(parts) == 1:
            return _native.decode_keys(keys[0])
        return _native.decode_keys(_native.merge_keys(keys) if k <= _native.MAX_FUSED_K else _native.merge_topk_keys(keys))

    # -- top-k distinct messages (tavb_search_top_messages_device per shard + tavb_merge_top_messages_host) ---------------------------
    @_locked
    def set_row_messages(self, row_to_message: np.ndarray, n_messages: int | None = None) -> None:
        """chunk row -> message ordinal for every row of the index (-1: none): every active shard gets its slice under the current
        `bounds` with the GLOBAL n_messages (None: the map's largest ordinal + 1) -- message ordinals stay global, nothing is remapped.
        The caller sets it again whenever the bounds change (`row_messages_bounds` says which bounds the slices were cut by)."""
        m = np.ascontiguousarray(row_to_message, dtype=np.int64).reshape(-1)
        if len(m) < self.rows:
            raise ValueError(f"the row -> message map covers {len(m)} rows, the index has {self.rows}")
        if n_messages is None:
            n_messages = int(m[: self.rows].max()) + 1 if self.rows else 0
        self.n_messages = max(int(n_messages), 0)
        for e, lo, hi in self._active():
            e.set_row_messages(m[lo:hi], self.n_messages)
        self.row_messages_bounds = tuple(self.bounds)

    def top_messages_capable(self) -> bool:
        """Every engine is a real `_native.Engine` (has the device-resident top-messages call) with the "top_messages" option on."""
        return all(hasattr(e, "search_top_messages_device") and e.get_option("top_messages") != 0 for e in self.engines)

    @_locked
    def search_top_messages(self, queries, k: int, thrs, handles=None):
        """`Engine.search_top_messages` over the shards: queries f32 [nq, dim]; thrs float32 [nq] (or one for all); 1 <= k <= MAX_LARGE_K;
        handles: None, or `mask_to_rows` under the current bounds -> (message ordinals [nq,k], scores [nq,k], counts [nq]).  Every shard
        returns its own best k messages (ONE tavb_search_top_messages_device per shard, all enqueued before any is waited for; under a
        mask only the shards with a handle are visited): a message of the whole-corpus top k is in the top k of the shard that holds its
        best row, with that score, so one maximum per message over the lists and the best k of those (tavb_merge_top_messages_host) is
        the whole-corpus answer.  Needs `set_row_messages` under the current bounds."""
        a = _native.batch_queries(queries, self.dim)
        nq = a.shape[0]
        t = _native.batch_thresholds(thrs, nq)
        if handles is None:
            parts = [(g, e, None) for g, e in enumerate(self.engines) if self.bounds[g + 1] > self.bounds[g]]
        else:
            if len(handles) != len(self.engines):
                raise ValueError("one handle (or None) per device")
            parts = [(g, e, handles[g]) for g, e in enumerate(self.engines) if handles[g] is not None and self.bounds[g + 1] > self.bounds[g]]
        if not parts or nq == 0:
            return np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        keys = self._on_all_parts(parts, a, k, lambda part, dq, out: part[1].search_top_messages_device(dq, k, t, out_keys=out, dev_rows=part[2]))
        return _native.decode_keys(keys[0] if len(parts) == 1 else _native.merge_top_messages_keys(keys))

    @_locked
    def search_all(self, q, thr: np.float32, max_out: int | None = None, subset_rows=None):
        """Every survivor, best first (one emit-all pass per shard, merged on the host)."""
        a = self._query(q)
        ids_all, sc_all = [], []
        rows = None if subset_rows is None else np.ascontiguousarray(subset_rows, dtype=np.int64)
        for e, lo, hi in self._active():
            if rows is None:
                i, s = e.search_all(a, thr, max_out)  # ordinals are global (ordinal_base = the shard's first row)
            else:
                idx = np.flatnonzero((rows >= lo) & (rows < hi))
                if idx.size == 0:
                    continue
                p, s = e.search_all(a, thr, max_out, subset_rows=rows[idx] - lo)
                i = idx[p]
            ids_all.append(i)
            sc_all.append(s)
        if not ids_all:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        ids, sc = np.concatenate(ids_all), np.concatenate(sc_all)
        order = np.lexsort((ids, -sc.astype(np.float64)))
        if max_out is not None:
            order = order[:max_out]
        return ids[order], sc[order]

    @_locked
    def search_subset(self, q, rows: np.ndarray, k: int, thr: np.float32):
        """rows: int64 global corpus row per subset position -> (positions int64[m], scores float32[m]); the order is
        (score desc, position asc) like one device's."""
        a = self._query(q)
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        pos_all, sc_all = [], []
        for e, lo, hi in self._active():
            idx = np.flatnonzero((rows >= lo) & (rows < hi))
            if idx.size == 0:
                continue
            p, s = e.search_subset(a, rows[idx] - lo, k, thr)
            pos_all.append(idx[p])
            sc_all.append(s)
        if not pos_all:
            return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
        pos = np.concatenate(pos_all)
        sc = np.concatenate(sc_all)
        order = np.lexsort((pos, -sc.astype(np.float64)))[:k]
        return pos[order], sc[order]
