"""GPU suite: the routes of the device-resident lookup, one table.

`tavb_search_device_dispatch` (csrc/tavb_route.hip) picks one of about ten routes for a batch: the grouped streaming scan, the streaming tiers
1-3 (8 queries per pass, 4 beyond k = 64), the 32/64-query tile (over the fp32 rows, or over the fp16 shadow of an fp32 corpus), the 128/256-query
tile with rescoring (fp16 rows, the fp32 shadow, the zero-padded copy of odd widths) and its exact fallbacks (the 64-query exact tile, the
split-plane form, for fp32 beyond k = 64 a re-run on the streaming kernels).  Every entry of ROUTES names the options that force one of them and
the getters that prove it was taken, and every route is checked the same way:

  (a) the getters after the call -- a route that silently changes fails instead of passing on another path;
  (b) full lists of sampled queries against the float64-refereed oracle, on a gaussian and an anisotropic corpus (min_score 0.85, where every row
      of a near query survives, and a threshold at the k/2-th score: near-ties at rank k), over the values the kernels multiply;
  (c) an output buffer poisoned with a valid-looking key (score 1.0, a real ordinal), on the device and in pinned host memory (what fused.py
      hands over): the answer equals the one written into a zeroed buffer bit for bit, in all nq x k slots;
  (d) a dense call then a sparse one into the same buffer: the second equals a fresh engine's answer;
  (e) ordinal bases 2^31 + 12345 and 2^32 - 2 - rows: the base-0 keys with every ordinal shifted, scores bit for bit, and two shards cut at an
      odd row merged on the device give the whole corpus' answer;
  (f) a mixed per-query threshold array through `search_batch`: query by query the single lookups with those thresholds.
The host-synchronous forms (h_out, h_lists, the host-merged direct forms, graph replay) have a table of their own below.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.synth import aniso_queries, make_aniso_corpus, make_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

BIG = 1 << 30
STREAM = (("direct_group_max_nq", 0), ("skinny_min_batch_f32", BIG), ("skinny_min_batch_f16", BIG))  # batches of 2 .. 8 stay on the streaming kernels
TILE = (("direct_group_max_nq", 0), ("mfma_min_batch_f32", BIG))  # the 32/64-query tile: no grouping, fp32 batches of 33+ not on the wide tile
SHADOW = TILE + (("f32_shadow", 2), ("f32_shadow_min_bytes", 0))
WIDE = (("direct_group_max_nq", 0),)  # (the grouped scan's cost model is not asked: these batches are the wide tile's)
FLAG = WIDE + (("band_max", 256),)
NQ_MAX = 256  # queries drawn per corpus; a route takes the first nq
POISON_ORD = 7  # (row 7 exists in every corpus here)


@dataclass(frozen=True)
class Route:
    name: str
    dtype: str
    rows: int
    dim: int
    nq: int
    k: int
    opts: tuple = ()
    expect: tuple = ()  # (getter, allowed values)
    kinds: tuple = ("gauss", "aniso")
    subset: bool = False
    stream_scores: bool = True  # the streaming kernels' float32 scores (tiers 1-3, grouped, rescored tiles): a batch equals its single lookups bit for bit
    planted: int = 0  # "planted" corpora: this many queries sit on 300 near-duplicates each (more than band_max = 256: flagged)


def T(tier, direct=0, shadow=None, flagged=None):
    e = [("last_tier", (tier,)), ("last_direct", (direct,))]
    if shadow is not None:
        e.append(("last_shadow", (shadow,)))
    if flagged is not None:
        e.append(("last_flagged", flagged))
    return tuple(e)


ROUTES = [
    # streaming tiers: 1 = D 1536 (one query; up to 4 forced), 2 = rows of whole 16-byte slices, 3 = anything else (fp16 D 100)
    Route("tier1-f32-q1", "fp32", 30_000, 1536, 1, 50, STREAM, T(1)),
    Route("tier1-f16-q1", "fp16", 30_000, 1536, 1, 50, STREAM, T(1)),
    Route("tier1-f32-q4-forced", "fp32", 30_000, 1536, 4, 32, STREAM + (("force_tier", 1),), T(1)),
    Route("tier2-f32-q8-d1536", "fp32", 30_000, 1536, 8, 50, STREAM, T(2)),
    Route("tier2-f32-q1-d384", "fp32", 60_000, 384, 1, 50, STREAM, T(2)),
    Route("tier2-f16-q6-d384", "fp16", 60_000, 384, 6, 64, STREAM, T(2)),
    Route("tier2-f32-q3-d100", "fp32", 60_000, 100, 3, 50, STREAM, T(2)),
    Route("tier3-f16-q1-d100", "fp16", 60_000, 100, 1, 50, STREAM, T(3)),
    Route("tier3-f16-q7-d100", "fp16", 60_000, 100, 7, 20, STREAM, T(3)),
    Route("tier3-f32-q3-forced", "fp32", 60_000, 100, 3, 50, STREAM + (("force_tier", 3),), T(3)),
    # k > 64: four queries per pass
    Route("per4-f16-q6-k100", "fp16", 60_000, 384, 6, 100, STREAM, T(2)),
    Route("per4-f32-q8-k100", "fp32", 30_000, 1536, 8, 100, STREAM, T(2)),  # (last_tier is the last pass': whole passes of 4)
    # grouped streaming scan (small corpora, 2 .. 128 queries): groups of 1 / 2 / 4 / 8 queries
    *[Route(f"grouped-f32-g{g}", "fp32", 5_000, 1536, 16, 32, (("direct_group", g),), T(1 if g == 1 else 2, 4)) for g in (1, 2, 4, 8)],
    Route("grouped-f16-g4", "fp16", 10_000, 1536, 20, 50, (("direct_group", 4),), T(2, 4)),
    # the 32/64-query tile
    Route("tile32-f32", "fp32", 40_000, 1536, 16, 50, TILE, T(5, shadow=0), stream_scores=False),
    Route("tile64-f32", "fp32", 40_000, 1536, 40, 64, TILE, T(5, shadow=0), stream_scores=False),
    Route("tile32-f16", "fp16", 40_000, 1536, 16, 50, TILE, T(5, shadow=0), stream_scores=False),
    Route("tile64-f16", "fp16", 40_000, 1536, 48, 32, TILE, T(5, shadow=0), stream_scores=False),
    # ... over the fp16 shadow of an fp32 corpus (level 2), rescored with the fp32 rows
    Route("shadow-tile-f32-q1", "fp32", 40_000, 1536, 1, 40, SHADOW, T(5, shadow=1)),
    Route("shadow-tile-f32-q16", "fp32", 40_000, 1536, 16, 48, SHADOW, T(5, shadow=1)),
    # the 128/256-query tile + rescoring
    Route("wide128-f16", "fp16", 40_000, 1536, 130, 50, WIDE + (("mfma_tile", 128),), T(4, shadow=0)),
    Route("wide256-f16", "fp16", 40_000, 1536, 130, 50, WIDE + (("mfma_tile", 256),), T(4, shadow=0)),
    Route("wide-f32-shadow", "fp32", 40_000, 1536, 70, 50, WIDE, T(4, shadow=1)),
    Route("wide-f16-odd-d100", "fp16", 60_000, 100, 70, 50, WIDE, T(4, shadow=1)),
    Route("wide-f16-odd-d1000", "fp16", 30_000, 1000, 70, 32, WIDE, T(4, shadow=1)),
    # k > 64 on the wide tile: fp16 flagged queries on the split-plane form, fp32 ones re-run on the streaming kernels
    *[Route(f"wide-{dt}-k{k}", dt, 40_000, 1536, 70, k, WIDE, T(4, shadow=int(dt == "fp32"))) for dt in ("fp16", "fp32") for k in (65, 256)],
    # flagged queries: bands that do not fit band_max = 256 (300 near-duplicates per planted query)
    Route("flagged-le64", "fp16", 60_000, 1536, 130, 32, FLAG, T(4, shadow=0, flagged=range(20, 65)), kinds=("planted",), planted=20),
    *[Route(f"flagged-gt64-wf{wf}-ee{ee}", "fp16", 60_000, 1536, 256, 32, FLAG + (("wide_fallback", wf), ("early_exact", ee)),
            T(4, shadow=0, flagged=range(65, 257)), kinds=("planted",), planted=100, stream_scores=wf == 1) for wf, ee in ((1, 1), (1, 0), (0, 0))],
    Route("flagged-f32-k100", "fp32", 40_000, 1536, 70, 100, FLAG, T(4, shadow=1, flagged=range(10, 71)), kinds=("planted",), planted=10),
    # subset of the corpus (keys carry subset positions)
    Route("subset-f32", "fp32", 30_000, 1536, 1, 50, (), T(1), subset=True),
    Route("subset-f16-d384", "fp16", 60_000, 384, 1, 50, (), T(2), subset=True),
]


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=3)
def _corpus(kind: str, rows: int, dim: int, dtype: str, planted: int = 0):
    """-> (the values the kernels multiply as float32 [rows, dim], the device tensor, queries [nq, dim])"""
    torch = _torch()
    seed = 7000 + dim + 7 * (kind == "aniso")
    if kind == "aniso":
        v = make_aniso_corpus(rows, dim, seed)
        q = aniso_queries(NQ_MAX, dim, seed)
        q[1::2] = make_queries(NQ_MAX, dim, seed + 1)[1::2]  # every other query is isotropic: nothing scores 0.85 for it
    else:
        v, _ = make_corpus(rows, dim, seed)
        q = make_queries(NQ_MAX, dim, seed + 1)
    if kind == "planted":
        rng = np.random.default_rng(seed + 2)
        ids = np.arange(1, 2 * planted, 2)  # odd queries sit on a cluster of near-duplicates
        where = rng.permutation(rows)[: planted * 300].reshape(planted, 300)
        for j, qi in enumerate(ids):
            base = q[qi] + 0.3 * rng.standard_normal(dim).astype(np.float32) / np.sqrt(dim)
            base /= np.linalg.norm(base)
            w = base[None, :] + 2e-4 * rng.standard_normal((300, dim)).astype(np.float32) / np.sqrt(dim)
            v[where[j]] = w / np.linalg.norm(w, axis=1, keepdims=True)
    if dtype == "fp16":
        v16 = v.astype(np.float16)
        return v16.astype(np.float32), torch.from_numpy(v16).cuda(), q
    return v, torch.from_numpy(v).cuda(), q


def _engine(route: Route, dev_corpus, rows=None, base: int = 0):
    eng = _native.Engine(0)
    for name, val in route.opts:
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev_corpus, rows=rows, ordinal_base=base)
    return eng


def _subset_rows(route: Route) -> np.ndarray:
    rng = np.random.default_rng(route.rows)
    s = rng.choice(route.rows, size=3000, replace=False)
    return np.concatenate([s, s[:40]])  # a row listed twice: two positions, two keys


def _lookup(eng, route: Route, dq, thr: float, out, d_rows=None):
    """one device-resident lookup into `out` (int64 [nq, k], device or pinned) -> a host copy of all nq x k keys"""
    torch = _torch()
    torch.cuda.synchronize()  # (the query / poison writes ran on torch's stream, the engine has a stream of its own)
    if route.subset:
        eng.search_subset_device(dq[0], d_rows, route.k, thr, out_keys=out)
    else:
        eng.search_device(dq, route.k, thr, out_keys=out)
    eng.synchronize()
    return out.cpu().numpy().copy()


def _buf(route: Route, fill: int = 0, pinned: bool = False):
    torch = _torch()
    nq = 1 if route.subset else route.nq
    if pinned:
        b = torch.empty((nq, route.k), dtype=torch.int64).pin_memory()
    else:
        b = torch.empty((nq, route.k), dtype=torch.int64, device="cuda")
    b.fill_(fill)
    return b


def _route_state(eng, route: Route) -> dict:
    return {g: eng.get_option(g) for g in ("last_tier", "last_direct", "last_shadow", "last_flagged", "last_graph")}


def _assert_route(eng, route: Route, what: str = "", expect=None):
    state = _route_state(eng, route)
    for getter, allowed in (route.expect if expect is None else expect):
        assert state[getter] in allowed, f"{route.name} {what}: {getter} = {state[getter]}, expected {list(allowed)[:6]} (all getters: {state})"


def _kth(v, q, k):
    s = np.sort(vo.scores_full(v, q))[::-1]
    return float(s[min(k // 2, len(s) - 1)])


def _thresholds(kind, v, qs, k):
    kth = _kth(v, qs[0], k)
    return {"gauss": [0.0, kth], "aniso": [0.85, kth], "planted": [0.0, kth]}[kind]


def _sampled(nq: int) -> list[int]:
    return sorted(set(i for i in (0, 1, 2, nq // 2, nq - 1) if i < nq))


def _check_oracle(route: Route, v, qs, keys, thr, sub=None):
    ords, scs, cnts = _native.decode_keys(keys)
    for qi in ([0] if route.subset else _sampled(route.nq)):
        m = int(cnts[qi])
        if sub is None:
            vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], route.k, thr, referee=vo.f64_referee(v, qs[qi]))
        else:
            vs = v[sub]
            vo.check_topk_parity(vo.scores_full(vs, qs[qi]), ords[qi, :m], scs[qi, :m], route.k, thr, referee=vo.f64_referee(vs, qs[qi]),
                                 candidate_ordinals=np.arange(len(sub)))
    return cnts


@pytest.mark.parametrize("route", ROUTES, ids=[r.name for r in ROUTES])
def test_device_route(route):
    torch = _torch()
    poison = _native.make_key(1.0, POISON_ORD)
    nq = 1 if route.subset else route.nq
    for kind in route.kinds:
        v, dev, qs_all = _corpus(kind, route.rows, route.dim, route.dtype, route.planted)
        qs = qs_all[:nq]
        dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
        sub = _subset_rows(route) if route.subset else None
        d_rows = torch.from_numpy(sub.astype(np.int32)).cuda() if route.subset else None
        eng = _engine(route, dev)
        thrs = _thresholds(kind, v if sub is None else v[sub], qs, route.k)
        answers = {}
        for thr in thrs:
            t32 = float(_native.f32_threshold(thr))
            # (a) + (b): a zeroed buffer
            zero = _lookup(eng, route, dq, t32, _buf(route), d_rows)
            _assert_route(eng, route, f"{kind} thr {thr}")
            cnts = _check_oracle(route, v, qs, zero, t32, sub)
            answers[thr] = zero
            # (c): poisoned with a valid-looking key, on the device and in pinned host memory
            for pinned in (False, True):
                got = _lookup(eng, route, dq, t32, _buf(route, poison, pinned), d_rows)
                assert not (got == poison).any(), f"{route.name} {kind} thr {thr}: a poison key survived (pinned={pinned})"
                np.testing.assert_array_equal(got, zero, err_msg=f"{route.name} {kind} thr {thr} pinned={pinned}")
            if thr == thrs[-1] and kind != "planted":
                assert cnts.min() < route.k, f"{route.name} {kind}: the sparse threshold left every query with k hits"
        # (d): dense then sparse into ONE reused buffer, same engine; the sparse answer is a fresh engine's
        out = _buf(route)
        dense = _lookup(eng, route, dq, float(_native.f32_threshold(thrs[0])), out, d_rows)
        if kind != "aniso":
            assert (_native.decode_keys(dense)[2] == route.k).all()
        sparse = _lookup(eng, route, dq, float(_native.f32_threshold(thrs[-1])), out, d_rows)
        fresh = _engine(route, dev)
        again = _lookup(fresh, route, dq, float(_native.f32_threshold(thrs[-1])), _buf(route), d_rows)
        np.testing.assert_array_equal(sparse, again, err_msg=f"{route.name} {kind}: stale keys after a dense call")
        np.testing.assert_array_equal(sparse, answers[thrs[-1]])
        fresh.close()
        if kind == route.kinds[0]:
            _check_bases(route, v, dev, dq, d_rows, float(_native.f32_threshold(thrs[0])), answers[thrs[0]])
            _check_batch_thresholds(route, eng, v, qs, thrs)
        eng.close()
        del dq, d_rows


def _shift(keys: np.ndarray, base: int) -> np.ndarray:
    """base-0 keys -> the keys of the same rows with ordinals + base (empty slots stay 0)"""
    k = keys.view(np.uint64)
    lo = np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)) + np.uint64(base)
    out = (k & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - lo)
    return np.where(k == 0, np.uint64(0), out).view(np.int64)


def _check_bases(route: Route, v, dev, dq, d_rows, thr: float, base0: np.ndarray):
    """(e): ordinals shifted by the base, scores bit for bit; two shards cut at an odd row, merged on the device, give the whole answer"""
    torch = _torch()
    for base in (2**31 + 12_345, 2**32 - 2 - route.rows):
        eng = _engine(route, dev, base=base)
        got = _lookup(eng, route, dq, thr, _buf(route), d_rows)
        _assert_route(eng, route, f"base {base}")
        want = base0 if route.subset else _shift(base0, base)  # (a subset's keys carry positions, whatever the base)
        np.testing.assert_array_equal(got, want, err_msg=f"{route.name}: ordinal base {base}")
        eng.close()
        if route.subset:
            continue
        cut = (route.rows // 2) | 1
        lists = torch.empty((2, route.nq, route.k), dtype=torch.int64, device="cuda")
        shards = []
        for lo, hi in ((0, cut), (cut, route.rows)):
            part = dev[lo:hi].clone()  # (its own allocation: 16-byte aligned like the whole, so the same kernels serve it)
            torch.cuda.synchronize()
            e = _engine(route, part, base=base + lo)
            e.search_device(dq, route.k, thr, out_keys=lists[len(shards)])
            e.synchronize()
            shards.append((e, part))
        merged = shards[0][0].merge_device(lists)
        shards[0][0].synchronize()
        np.testing.assert_array_equal(merged.cpu().numpy(), want, err_msg=f"{route.name}: two shards at base {base} merged")
        for e, _ in shards:
            e.close()


def _check_batch_thresholds(route: Route, eng, v, qs, thrs):
    """(f): one threshold per query through search_batch == the single lookups with those thresholds"""
    if route.subset:
        return
    nq = route.nq
    t = np.empty(nq, dtype=np.float32)
    pattern = [thrs[0], thrs[-1], float("nan"), 1.5, thrs[0] + (thrs[-1] - thrs[0]) / 2]
    for i in range(nq):
        t[i] = _native.f32_threshold(pattern[i % len(pattern)])
    if nq == 1:
        t[0] = _native.f32_threshold(thrs[-1])
    ords, scs, cnts = eng.search_batch(qs, route.k, t)
    if nq > 8:  # (smaller batches on small corpora take the host-merged direct forms; the grouped scan its host-merged form, last_direct 3;
        #          fewer queries are flagged when some thresholds admit nothing)
        host = tuple((g, (3,) if g == "last_direct" and 4 in a else a) for g, a in route.expect if g != "last_flagged")
        _assert_route(eng, route, "search_batch with per-query thresholds", host)
    for qi in _sampled(nq) + [min(3, nq - 1), min(4, nq - 1)]:
        m = int(cnts[qi])
        if t[qi] != t[qi] or t[qi] > 1:
            assert m == 0
            continue
        so, ss = eng.search(qs[qi], route.k, t[qi])
        if route.stream_scores:
            assert ords[qi, :m].tolist() == so.tolist() and scs[qi, :m].tolist() == ss.tolist(), (route.name, qi)
        else:  # the 32/64-query tile's own accumulation order: within float32 noise of the streaming kernel's; the referee decides the rest
            assert m == len(so) or abs(m - len(so)) <= 1, (route.name, qi, m, len(so))
            vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], route.k, float(t[qi]), referee=vo.f64_referee(v, qs[qi]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# host-synchronous forms: h_out (the dispatch's keys in pinned memory), h_lists (the host-merged direct forms), graph replay
HOST_ROUTES = [
    Route("host-direct-inline", "fp32", 10_000, 1536, 1, 50, (), (("last_direct", (2,)),)),
    Route("host-direct-copy", "fp32", 10_000, 1536, 1, 50, (("inline_query", 0),), (("last_direct", (1,)),)),
    Route("host-direct-few", "fp32", 3_000, 384, 6, 50, (("direct_group_max_nq", 0),), (("last_direct", (1,)),)),
    Route("host-direct-grouped", "fp32", 5_000, 1536, 16, 32, (("direct_group", 2),), (("last_direct", (3,)),)),
    Route("host-dispatch-stream", "fp32", 10_000, 1536, 1, 50, (("small_direct_bytes", 0),), T(1)),
    Route("host-dispatch-tile", "fp32", 40_000, 1536, 16, 50, TILE, T(5, shadow=0)),
    Route("host-dispatch-wide", "fp16", 40_000, 1536, 130, 50, WIDE, T(4, shadow=0)),
    Route("host-graph", "fp32", 10_000, 1536, 1, 50, (("graph_max_bytes", 256 << 20),), (("last_graph", (1,)),)),
]


def _host_call(eng, route: Route, qs, thr: float):
    if route.nq == 1:
        o, s = eng.search(qs[0], route.k, np.float32(thr))
        return o[None, :], s[None, :], np.array([len(o)], dtype=np.int32)
    return eng.search_batch(qs, route.k, np.float32(thr))


@pytest.mark.parametrize("route", HOST_ROUTES, ids=[r.name for r in HOST_ROUTES])
def test_host_route_dense_then_sparse(route):
    """(d) through search / search_batch: a sparse call after a dense one of the same shape on the same engine returns a fresh engine's answer."""
    v, dev, qs_all = _corpus("gauss", route.rows, route.dim, route.dtype)
    qs = qs_all[: route.nq]
    dense_t, sparse_t = 0.0, float(_native.f32_threshold(_kth(v, qs[0], route.k)))
    eng = _engine(route, dev)
    graph = route.name == "host-graph"

    def run(thr):
        for _ in range(4 if graph else 1):  # a graph is captured on the second call of a shape and replayed from then on
            r = _host_call(eng, route, qs, thr)
            if not graph or eng.get_option("last_graph") == 1:
                break
        _assert_route(eng, route, f"thr {thr}")
        return r

    o, s, c = run(dense_t)
    assert (c == route.k).all()
    o, s, c = run(sparse_t)
    assert c.min() < route.k
    if graph:  # the replay again, after a capture of the dense shape in between
        run(dense_t)
        o, s, c = run(sparse_t)
    fresh = _engine(route, dev)
    fo, fs, fc = _host_call(fresh, route, qs, sparse_t)
    np.testing.assert_array_equal(c, fc)
    for qi in range(route.nq):
        m = int(c[qi])
        assert o[qi, :m].tolist() == fo[qi, :m].tolist() and s[qi, :m].tolist() == fs[qi, :m].tolist(), (route.name, qi)
    for qi in _sampled(route.nq):
        m = int(c[qi])
        vo.check_topk_parity(vo.scores_full(v, qs[qi]), o[qi, :m], s[qi, :m], route.k, sparse_t, referee=vo.f64_referee(v, qs[qi]))
    fresh.close()
    eng.close()
