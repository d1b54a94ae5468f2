"""GPU suite: every lookup route on un-normalised, out-of-range and non-finite QUERIES (the table: tests/query_edge_cases.py; its CPU twin:
tests/test_query_edge_cases_host.py).  One test per route; a test runs all of its batches, checks every query of every batch and names every
failure:

  * the answer against the float64-refereed oracle, scores in [0, 1], item for item where the table calls the query exact (`check_answer`);
  * counts within [0, k];
  * the route state (`last_tier`, `last_shadow`, `last_flagged`, `last_direct`): a batch without an out-of-range query must take the route
    under test; one WITH an element that rounds to an fp16 infinity or NaN must leave the tiles for the streaming kernels (tiers 1-3), which
    is how the host-synchronous entry points keep such queries exact (csrc/tavb_ctx.h `staged_overflow`);
  * batch == sequential: the answer of every query equals `search` of that query alone -- item for item always, score bits too on the routes
    DESIGN calls bit-identical to the scan (grouped, the wide path after rescoring, large k, sorted) and whenever the table calls the query
    exact; the 32/64-query tile's own scores are compared through the referee;
  * `last_direct` on the grouped routes, `last_skinny_kernel` (32- or 64-query tile) on the tile routes;
  * on the two flagged routes (band_max = 256) `last_flagged` is at least the number of queries with more than 256 rows tied exactly at
    their k-th best score (read off the oracle: scores clipped to 1.0, the zero query's 0.5), at most 64 on `flagged-le64`, and one batch
    of `flagged-gt64` has more than 64 of them; with `scale-50` in a filter batch the count is also recorded in the failure text
    (queries with delta = inf no longer reach the filter);
  * the raw key arrays of the dispatch (tavb_search_begin / _end) over a poisoned buffer: sorted, zero past the count, the same answer.
`test_class_overflow_queries` runs the out-of-range kinds through `VectorBase.fuzzy_lookup_embeddings` / `fuzzy_lookup_embedding`.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import pytest

from tests import query_edge_cases as qc
from tests.test_gpu_routes import FLAG, SHADOW, STREAM, TILE, WIDE
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

NO_DIRECT = (("small_direct_bytes", 0),)  # (700 rows: without it a host batch of up to 8 queries takes the one-launch scan)
SCAN_TIERS = (1, 2, 3)
LEAVES_TILES = qc.OVERFLOW_KINDS + qc.NONFINITE_KINDS  # an element whose fp16 rounding is not finite: the batch runs on the streaming kernels


@dataclass(frozen=True)
class Route:
    name: str
    dtype: str
    dim: int
    nq: int
    k: int
    opts: tuple = ()
    call: str = "batch"  # batch, single, topk, sorted, masked, scoped_tile, top_messages, top_messages_tile
    tier: tuple = ()  # allowed last_tier of a batch without out-of-range queries
    shadow: object = None
    flagged: str = ""  # "le64" / "gt64": the exact fallback the flagged queries of the filter must take (band_max = 256)
    direct: tuple = ()  # allowed last_direct of the host batch
    qt: int = 0  # queries per tile of the 32/64-query tile: last_skinny_kernel % 100
    bits: bool = True  # a batch equals its single lookups in score bits too
    few: bool = False  # only FEW_KINDS
    ckinds: tuple = ("gauss", "gauss-z")


ROUTES = [
    Route("scan-tier1-f32", "fp32", 1536, 24, 10, STREAM, "single", (1,)),
    Route("scan-tier1-f16", "fp16", 1536, 24, 64, STREAM, "single", (1,)),
    Route("scan-tier2-f32-d64", "fp32", 64, 24, 100, STREAM, "single", (2,)),
    Route("scan-tier2-f16-d200-k1", "fp16", 200, 24, 1, STREAM, "single", (2,)),
    Route("scan-tier3-f16-d200", "fp16", 200, 24, 10, STREAM + (("force_tier", 3),), "single", (3,)),
    Route("grouped-f32", "fp32", 1536, 16, 10, (("direct_group", 2),), "batch", (2,), direct=(3,)),
    Route("grouped-f16-d64", "fp16", 64, 34, 64, (("direct_group", 4),), "batch", (2,), direct=(3,)),
    Route("tile32-f32", "fp32", 1536, 16, 10, TILE + NO_DIRECT, "batch", (5,), 0, bits=False, qt=32),
    Route("tile64-f32-d64", "fp32", 64, 40, 64, TILE + NO_DIRECT, "batch", (5,), 0, bits=False, qt=64),
    Route("tile32-f16-k1", "fp16", 1536, 16, 1, TILE + NO_DIRECT, "batch", (5,), 0, bits=False, qt=32),
    Route("tile64-f16-d64", "fp16", 64, 48, 64, TILE + NO_DIRECT, "batch", (5,), 0, bits=False, qt=64),
    Route("wide128-f16", "fp16", 1536, 130, 10, WIDE + NO_DIRECT + (("mfma_tile", 128),), "batch", (4,), 0),
    Route("wide256-f16-d64", "fp16", 64, 130, 64, WIDE + NO_DIRECT + (("mfma_tile", 256),), "batch", (4,), 0),
    Route("wide-f16-d200-k1", "fp16", 200, 70, 1, WIDE + NO_DIRECT, "batch", (4,), 1),
    Route("wide-f16-k100", "fp16", 1536, 70, 100, WIDE + NO_DIRECT, "batch", (4,), 0),
    Route("wide-f32-shadow", "fp32", 1536, 70, 10, WIDE + NO_DIRECT, "batch", (4,), 1),
    Route("shadow-tile-f32", "fp32", 1536, 16, 10, SHADOW + NO_DIRECT, "batch", (5,), 1),
    Route("flagged-le64", "fp16", 1536, 100, 10, FLAG + NO_DIRECT, "batch", (4,), 0, flagged="le64"),
    Route("flagged-gt64", "fp16", 1536, 256, 10, FLAG + NO_DIRECT, "batch", (4,), 0, flagged="gt64"),
    Route("topk-k300-f16", "fp16", 1536, 12, 300, (), "topk"),
    Route("topk-k300-f32-d64", "fp32", 64, 12, 300, (), "topk"),
    Route("sorted-f16", "fp16", 1536, 12, 0, (), "sorted"),
    Route("sorted-f32-d64", "fp32", 64, 12, 0, (), "sorted"),
    Route("masked-tile-f16", "fp16", 1536, 16, 10, (), "masked", (5,), few=True),
    Route("scoped-tile-f16", "fp16", 1536, 16, 10, (), "scoped_tile", (5,), few=True, bits=False),
    Route("masked-wide-f16", "fp16", 1536, 130, 10, (), "masked_wide", (4,), few=True),
    Route("scoped-wide-f16", "fp16", 1536, 130, 10, (), "scoped_wide", (4,), few=True),
    Route("top-messages-f16", "fp16", 1536, 12, 10, (), "top_messages", few=True),
    Route("top-messages-tile-f16", "fp16", 1536, 16, 10, (), "top_messages_tile", (5,), few=True, bits=False),
    Route("top-messages-tile-nomask-f16", "fp16", 1536, 16, 10, (), "top_messages_tile_all", (5,), few=True, bits=False),
]


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=4)
def _device_corpus(ckind: str, dim: int, dtype: str):
    return _torch().from_numpy(np.array(qc.corpus(ckind, dim, dtype)[1])).cuda()


def _allowed() -> np.ndarray:
    m = np.ones(qc.ROWS, dtype=bool)
    m[[0, 1, 9, 300, 301, 697]] = False  # (none of the planted rows)
    return m


def _kinds(route: Route, ckind: str, overflow: bool) -> tuple:
    kinds = qc.FEW_KINDS if route.few else qc.kinds_for(ckind)
    if route.call == "sorted":
        kinds = tuple(k for k in kinds if k != "scale-1000")  # (dropped at k = 0: tests/query_edge_cases.py host_cases)
    if route.name.startswith("flagged"):
        # kept out: at ||q|| = 2^-20 every element is below fp16's smallest subnormal, the exact fallbacks' planes hi + lo carry q only to
        # 2^-25 absolute, and their choice among rows within one float32 ulp of 0.5 differs from the scan's
        kinds = tuple(k for k in kinds if k != "scale-2^-20")
    return tuple(k for k in kinds if overflow or k not in LEAVES_TILES)


def _run(eng, route: Route, qs, thrs, mask_bits, mask_rows=None):
    """-> per query (items, scores)"""
    nq, k = qs.shape[0], route.k
    if route.call == "single":
        return [eng.search(qs[i], k, np.float32(thrs[i])) for i in range(nq)]
    if route.call == "sorted":
        o, s, c = eng.search_sorted(qs, 0, thrs)
        off = np.concatenate([[0], np.cumsum(c)])
        return [(o[off[i]:off[i + 1]], s[off[i]:off[i + 1]]) for i in range(nq)]
    if route.call == "topk":
        o, s, c = eng.search_topk(qs, k, thrs)
    elif route.call == "masked":
        o, s, c = eng.search_masked_batch(qs, mask_bits, k, thrs)
    elif route.call == "masked_wide":
        o, s, c = eng.search_masked_wide(qs, mask_bits, mask_rows, k, thrs)
    elif route.call == "scoped_tile":
        o, s, c = eng.search_scoped_tile(qs, [mask_bits] * nq, k, thrs)
    elif route.call == "scoped_wide":
        o, s, c = eng.search_scoped_wide(qs, [mask_bits] * nq, k, thrs)
    elif route.call == "top_messages_tile_all":
        o, s, c = eng.search_top_messages_tile(qs, k, thrs)
    elif route.call == "top_messages":
        o, s, c = eng.search_top_messages(qs, k, thrs)
    elif route.call == "top_messages_tile":
        o, s, c = eng.search_top_messages_tile(qs, k, thrs, dev_bits=mask_bits)
    else:
        o, s, c = eng.search_batch(qs, k, thrs)
    assert ((c >= 0) & (c <= k)).all(), f"counts outside [0, {k}]: {c.tolist()}"
    return [(o[i, : int(c[i])], s[i, : int(c[i])]) for i in range(nq)]


def _raw_keys(eng, route: Route, qs, thrs, got, what: str, failures: list) -> None:
    """the same batch through tavb_search_begin / _end, which hand out the RAW key arrays [nq, k] of the dispatch: sorted, zero-padded
    past each query's count, and -- decoded -- the answer `search_batch` gave, item for item and bit for bit"""
    nq, k = qs.shape[0], route.k
    keys = np.full((nq, k), 0x3F80000000000007, dtype=np.uint64)  # (poison: score 1.0, ordinal 0xFFFFFFF8)
    eng.search_begin(np.ascontiguousarray(qs), k, np.ascontiguousarray(thrs))
    eng.search_end(nq, k, keys)
    ords, scs, cnts = _native.decode_keys(keys.view(np.int64))
    for i in range(nq):
        m = int(cnts[i])
        if (keys[i, m:] != 0).any() or (keys[i, :m] == 0).any():
            failures.append(f"{what} q{i}: raw keys not zero-padded past the count {m}: {keys[i].tolist()[:12]}")
        elif keys[i, :m].tolist() != sorted(set(keys[i, :m].tolist()), reverse=True):
            failures.append(f"{what} q{i}: raw keys not strictly descending")
        elif ords[i, :m].tolist() != np.asarray(got[i][0]).tolist() or scs[i, :m].tolist() != np.asarray(got[i][1]).tolist():
            failures.append(f"{what} q{i}: the raw keys decode to another answer than search_batch's")


def _sure_flagged(v, qs, thrs, k: int, band_max: int = 256) -> int:
    """queries the filter MUST flag, read off the oracle: more than band_max rows tie exactly with the k-th best passing score (clipped
    to 1.0, or 0.5 under the zero query), so no band of band_max keys holds them whatever delta is"""
    n = 0
    for q, thr in zip(qs, thrs):
        ref = qc.oracle_scores(v, q)
        with np.errstate(invalid="ignore"):
            ok = np.sort(ref[ref >= np.float32(thr)])[::-1]
        if ok.size >= k and int((ok == ok[k - 1]).sum()) > band_max:
            n += 1
    return n


def _single(ref, route: Route, q, thr):
    """the sequential lookup of one query: `search` (beyond the fused k: `search_all`) on an engine with default options"""
    if route.call in ("topk", "sorted"):
        return ref.search_all(q, np.float32(thr), max_out=route.k if route.k else None)
    return ref.search(q, route.k, np.float32(thr))


@pytest.mark.parametrize("route", ROUTES, ids=[r.name for r in ROUTES])
def test_query_edges(route):
    torch = _torch()
    failures, notes = [], []
    masked = route.call in ("masked", "masked_wide", "scoped_tile", "scoped_wide", "top_messages_tile")
    flagged_seen = []
    allowed = _allowed() if masked else None
    for ckind in route.ckinds:
        v, _ = qc.corpus(ckind, route.dim, route.dtype)
        dev = _device_corpus(ckind, route.dim, route.dtype)
        eng = _native.Engine(0)
        for name, val in route.opts:
            eng.set_option(name, val)
        eng.set_corpus_tensor(dev)
        ref = _native.Engine(0)  # the sequential lookups: default options, one query at a time
        ref.set_corpus_tensor(dev)
        mask_rows, _, mask_bits = eng.mask_to_rows_bits(allowed) if masked else (None, 0, None)
        if route.call.startswith("top_messages"):
            eng.set_row_messages(np.arange(qc.ROWS, dtype=np.int32))  # one message per row: the best messages are the best rows
            if route.call == "top_messages_tile":
                eng.set_option("top_messages_tile", 2)
        for label, overflow, all_edge in (("mixed", False, False), ("with-overflow", True, False), ("all-edge", False, True)):
            kinds = _kinds(route, ckind, overflow)
            qs, thrs, slots = qc.batch(ckind, route.dim, route.dtype, route.nq, kinds, route.k, all_edge=all_edge)
            what = f"{route.name} {ckind} {label}"
            try:
                got = _run(eng, route, qs, thrs, mask_bits, mask_rows)
            except Exception as e:  # noqa: BLE001 -- name the batch, go on with the next
                failures.append(f"{what}: {type(e).__name__}: {e}")
                continue
            state = {g: eng.get_option(g) for g in ("last_tier", "last_shadow", "last_flagged", "last_direct", "last_skinny_kernel")}
            has_over = any(s.kind in LEAVES_TILES for s in slots)
            tiles = bool(route.tier) and route.tier[0] in (4, 5)
            if tiles and has_over:
                if state["last_tier"] not in SCAN_TIERS:
                    failures.append(f"{what}: an out-of-range query stayed on the tiles ({state})")
            elif route.tier and state["last_tier"] not in route.tier:
                failures.append(f"{what}: last_tier {state['last_tier']}, expected {route.tier} ({state})")
            if route.shadow is not None and not has_over and state["last_shadow"] != route.shadow:
                failures.append(f"{what}: last_shadow {state['last_shadow']}, expected {route.shadow}")
            if route.direct and state["last_direct"] not in route.direct:
                failures.append(f"{what}: last_direct {state['last_direct']}, expected {route.direct}")
            if route.qt and not has_over and state["last_skinny_kernel"] % 100 != route.qt:
                failures.append(f"{what}: last_skinny_kernel {state['last_skinny_kernel']}, expected the {route.qt}-query tile")
            if route.flagged and not has_over:
                sure = _sure_flagged(v, qs, thrs, route.k)
                flagged_seen.append((sure, state["last_flagged"]))
                if state["last_flagged"] < sure or state["last_flagged"] > route.nq:
                    failures.append(f"{what}: last_flagged {state['last_flagged']}, at least {sure} queries tie beyond band_max")
                if route.flagged == "le64" and state["last_flagged"] > 64:
                    failures.append(f"{what}: last_flagged {state['last_flagged']} > 64: not the 64-query exact tile")
            if any(s.kind == "scale-50" for s in slots) and route.tier == (4,) and not has_over:
                notes.append(f"{what}: last_flagged {state['last_flagged']} with scale-50 in the batch")
            if route.call == "batch":
                _raw_keys(eng, route, qs, thrs, got, what, failures)
            for i, (items, scores) in enumerate(got):
                q, thr, kind = qs[i], float(thrs[i]), slots[i].kind
                tag = f"{what} q{i} {kind} thr {thr}"
                exact = qc.is_exact(v, q)
                try:
                    vm = v
                    if allowed is not None:
                        vm = v.copy()
                        vm[~allowed] = np.nan  # a NaN row never passes and is never looked at by the referee
                    qc.check_answer(vm, q, items, scores, route.k, thr, exact, tag)
                except AssertionError as e:
                    failures.append(f"{tag}: {str(e)[:300]}")
                    continue
                if allowed is not None or route.call == "single":
                    continue  # (the sequential form of a masked lookup is the oracle over the allowed rows, checked above; a single lookup is its own)
                so, ss = _single(ref, route, q, thr)
                if items.tolist() != so.tolist():
                    if route.bits or exact:
                        failures.append(f"{tag}: batch != sequential: items {items.tolist()[:8]} vs {so.tolist()[:8]} ({len(items)} / {len(so)})")
                    else:  # the tile's own accumulation order: the sequential answer must pass the same referee
                        try:
                            qc.check_answer(v, q, so, ss, route.k, thr, exact, tag + " (sequential)")
                        except AssertionError as e:
                            failures.append(f"{tag}: sequential answer: {str(e)[:300]}")
                elif (route.bits or exact) and np.asarray(scores).tolist() != np.asarray(ss).tolist():
                    failures.append(f"{tag}: batch != sequential: score bits differ")
        eng.close()
        ref.close()
    torch.cuda.synchronize()
    if route.flagged == "le64" and not any(1 <= sure for sure, _ in flagged_seen):
        failures.append(f"{route.name}: no batch had a query that must be flagged ({flagged_seen})")
    if route.flagged == "gt64" and not any(sure > 64 and got_n > 64 for sure, got_n in flagged_seen):
        failures.append(f"{route.name}: no batch had more than 64 queries that must be flagged ({flagged_seen})")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:60]) + ("\nnotes:\n" + "\n".join(notes) if notes else "")


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_class_overflow_queries(dtype):
    """the class: a batch with out-of-range and non-finite queries among unit ones equals its single lookups item for item and bit for
    bit, and both are the oracle's answer (40 queries: the class sends the batch to the 32/64-query tile route when nothing is wrong)"""
    from tests.fakes import NullModel
    from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase

    v, _ = qc.corpus("gauss-z", 1536, dtype)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    vb.add_embeddings(None, np.ascontiguousarray(qc.corpus("gauss-z", 1536, "fp32")[0]))
    failures = []
    for k in (1, 10):
        qs, thrs, slots = qc.batch("gauss-z", 1536, dtype, 40, LEAVES_TILES + ("scale-50", "zero"), k)
        batch = vb.fuzzy_lookup_embeddings(qs, max_hits=k, min_score=thrs)
        assert len(batch) == 40
        for i, res in enumerate(batch):
            tag = f"class {dtype} k{k} q{i} {slots[i].kind} thr {float(thrs[i])}"
            items, scores = [r.item for r in res], [r.score for r in res]
            one = vb.fuzzy_lookup_embedding(qs[i], max_hits=k, min_score=float(thrs[i]))
            if items != [r.item for r in one] or scores != [r.score for r in one]:
                failures.append(f"{tag}: batch != sequential: {items[:8]} vs {[r.item for r in one][:8]}")
            try:
                qc.check_answer(v, qs[i], items, scores, k, float(thrs[i]), qc.is_exact(v, qs[i]), tag)
            except AssertionError as e:
                failures.append(f"{tag}: {str(e)[:300]}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures[:40])
