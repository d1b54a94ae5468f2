"""GPU suite: FusedIndexQuery (one submission for the T term lookups, the message re-rank and the thread lookup of a user question) on
anisotropic corpora, where min_score 0.85 keeps most rows of a near query and its k = 50 lists are selections among thousands of survivors.

Covers the term-batch sizes that change the route of the terms lookup (T = 1, 2 .. 4, 5+, 33+, 65+), fp32 and fp16 corpora at the reference's
scale and at 200k rows, subsets with survivors / negative / duplicate ordinals / nothing, buffer reuse across calls of one shape (dense then
sparse, T changed, a lookup dropped and put back), subclasses and instances with other K attributes, and a bad subset."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.synth import aniso_queries, make_aniso_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

DIM = 1536
T_VALUES = (1, 2, 4, 5, 8, 32, 33, 64, 128)


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=2)
def _terms(rows: int, dtype: str):
    torch = _torch()
    v = make_aniso_corpus(rows, DIM, 9300 + rows % 97)
    if dtype == "fp16":
        v = v.astype(np.float16)
        return v.astype(np.float32), torch.from_numpy(v).cuda(), 9300 + rows % 97
    return v, torch.from_numpy(v).cuda(), 9300 + rows % 97


@functools.lru_cache(maxsize=1)
def _side():
    """messages (20k rows) and threads (1000 rows), fp32, anisotropic; near queries for both"""
    torch = _torch()
    msgs = make_aniso_corpus(20_000, DIM, 9401)
    thr = make_aniso_corpus(1_000, DIM, 9402)
    return msgs, thr, torch.from_numpy(msgs).cuda(), torch.from_numpy(thr).cuda(), aniso_queries(4, DIM, 9401), aniso_queries(4, DIM, 9402)


def _fused(terms_dev, cls=None):
    from typeagent_py_amd.fused import FusedIndexQuery

    fq = (cls or FusedIndexQuery)(0)
    _, _, mdev, hdev, _, _ = _side()
    fq.set_corpus("terms", terms_dev)
    fq.set_corpus("messages", mdev)
    fq.set_corpus("threads", hdev)
    _torch().cuda.synchronize()
    return fq


def _pairs(hits):
    return [(h.item, h.score) for h in hits]


def _check(v, q, hits, k, ms, subset=None):
    items = [h.item for h in hits]
    scores = [h.score for h in hits]
    if subset is None:
        vo.check_topk_parity(vo.scores_full(v, q), items, scores, k, ms, referee=vo.f64_referee(v, q))
    else:
        rows = np.where(np.asarray(subset) < 0, np.asarray(subset) + len(v), np.asarray(subset))
        vs = v[rows]
        vo.check_topk_parity(vo.scores_full(vs, q), items, scores, k, ms, referee=vo.f64_referee(vs, q), candidate_ordinals=np.asarray(subset))


def _single(v_dev, q, k, ms, subset_rows=None):
    """the separate lookup (what VectorBase.fuzzy_lookup_embedding asks the engine for)"""
    eng = _native.Engine(0)
    eng.set_corpus_tensor(v_dev)
    if subset_rows is None:
        o, s = eng.search(q, k, _native.f32_threshold(ms))
    else:
        o, s = eng.search_subset(q, np.asarray(subset_rows, dtype=np.int64), k, _native.f32_threshold(ms))
    eng.close()
    return list(zip(o.tolist(), s.tolist()))


def _tq(T: int, seed: int, far_every: int = 0):
    q = aniso_queries(T, DIM, seed)
    if far_every:
        q[1::far_every] = make_queries(T, DIM, seed + 5)[1::far_every]
    return q


@pytest.mark.parametrize("rows,dtype", [(1294, "fp32"), (10_000, "fp16"), (10_000, "fp32"), (200_000, "fp16"), (200_000, "fp32")])
def test_fused_terms_routes_against_the_oracle(rows, dtype):
    """every T of T_VALUES: the terms batch takes the route search_device takes for it, full 50-long lists are the oracle's, and item for item
    the separate lookups' (the 32/64-query tile has its own accumulation order: within float32 noise there, judged by the referee)"""
    torch = _torch()
    v, dev, seed = _terms(rows, dtype)
    fq = _fused(dev)
    probe = _native.Engine(0)
    probe.set_corpus_tensor(dev)
    for T in T_VALUES:
        tq = _tq(T, seed)
        res = fq.run(tq)
        route = (fq.engine.get_option("last_tier"), fq.engine.get_option("last_direct"))
        assert len(res.terms) == T and res.messages == [] and res.threads == []
        dq = torch.from_numpy(tq).cuda()
        torch.cuda.synchronize()
        probe.search_device(dq, 50, float(_native.f32_threshold(0.85)))
        probe.synchronize()
        assert route == (probe.get_option("last_tier"), probe.get_option("last_direct")), (rows, dtype, T)
        if T == 1:
            assert route[0] in (1, 2, 3)
        elif T >= 65 and dtype == "fp16":
            assert route[0] == 4 or route[1] == 4, (T, route)
        assert route[0] in (1, 2, 3, 4, 5)
        for i in sorted(set([0, T // 2, T - 1])):
            hits = res.terms[i]
            assert len(hits) == min(50, rows)  # (min_score 0.85 keeps every row of a near query)
            _check(v, tq[i], hits, 50, 0.85)
            single = _single(dev, tq[i], 50, 0.85)
            if route[0] != 5:
                assert _pairs(hits) == single, (rows, dtype, T, i)
            else:  # (float32 accumulation of DIM terms in another order: on these rows, scores ~0.89, up to 4.2e-7 apart was measured)
                assert len(hits) == len(single)
                np.testing.assert_allclose([h.score for h in hits], [s for _, s in single], atol=vo.fp32_accumulation_scale(DIM), rtol=0)
    probe.close()


def test_fused_messages_threads_subset_and_buffer_reuse():
    v, dev, seed = _terms(10_000, "fp16")
    msgs, thr, mdev, hdev, mq, hq = _side()
    fq = _fused(dev)
    tq = _tq(8, seed, far_every=2)  # odd term queries are isotropic: no row reaches 0.85 for them
    full = fq.run(tq, mq[0], hq[0])
    for i in range(8):
        assert len(full.terms[i]) == (50 if i % 2 == 0 else 0)
        _check(v, tq[i], full.terms[i], 50, 0.85)
    assert len(full.messages) == 25 and len(full.threads) == 10
    _check(msgs, mq[0], full.messages, 25, 0.7)
    _check(thr, hq[0], full.threads, 10, 0.7)
    assert _pairs(full.messages) == _single(mdev, mq[0], 25, 0.7) and _pairs(full.threads) == _single(hdev, hq[0], 10, 0.7)
    # subsets: survivors, negative and duplicate ordinals; an empty one
    rng = np.random.default_rng(9500)
    subset = rng.choice(20_000, 3000, replace=False).tolist()
    subset += [-1, -20_000, subset[0], subset[1]]
    sub = fq.run(tq, mq[0], hq[0], message_subset=subset)
    rows = [s % 20_000 for s in subset]
    assert len(sub.messages) == 25
    _check(msgs, mq[0], sub.messages, 25, 0.7, subset=subset)
    want = [(subset[p], s) for p, s in _single(mdev, mq[0], 25, 0.7, subset_rows=rows)]
    assert _pairs(sub.messages) == want
    assert [_pairs(t) for t in sub.terms] == [_pairs(t) for t in full.terms] and _pairs(sub.threads) == _pairs(full.threads)
    empty = fq.run(tq, mq[0], hq[0], message_subset=[])
    assert empty.messages == [] and _pairs(empty.threads) == _pairs(full.threads)
    # dense then sparse, same shape: every term query far, the message query far, no thread query
    far = make_queries(8, DIM, 9501)
    sparse = fq.run(far, far[0], None)
    assert all(t == [] for t in sparse.terms) and sparse.messages == [] and sparse.threads == []
    # T changes between calls; a lookup dropped and put back
    r3 = fq.run(tq[:3], mq[1], hq[1])
    assert [_pairs(t) for t in r3.terms] == [_pairs(t) for t in full.terms[:3]]
    assert _pairs(r3.messages) == _single(mdev, mq[1], 25, 0.7) and _pairs(r3.threads) == _single(hdev, hq[1], 10, 0.7)
    no_msg = fq.run(tq[:3], None, hq[1])
    assert no_msg.messages == [] and _pairs(no_msg.threads) == _pairs(r3.threads)
    back = fq.run(tq[:3], mq[1], hq[1])
    assert _pairs(back.messages) == _pairs(r3.messages)
    again = fq.run(tq, mq[0], hq[0])
    assert [_pairs(t) for t in again.terms] == [_pairs(t) for t in full.terms] and _pairs(again.messages) == _pairs(full.messages)
    # a fresh instance answers the sparse call the same way
    assert fq.run(far, far[0], None) == _fused(dev).run(far, far[0], None)


def test_fused_k_attributes():
    """k beyond 64 for the messages (another single-query route), THREADS_K above TERMS_K, and K attributes changed on an instance between two
    runs of the same shape: the terms lists stay in their rows, nothing is written past the result buffer, the answers are the oracle's"""
    from typeagent_py_amd.fused import FusedIndexQuery

    class Wide(FusedIndexQuery):
        MESSAGES_K = 100
        THREADS_K = 60

    v, dev, seed = _terms(10_000, "fp32")
    msgs, thr, mdev, hdev, mq, hq = _side()
    tq = _tq(5, seed)
    for fq in (_fused(dev, Wide), _fused(dev)):
        if type(fq) is FusedIndexQuery:
            fq.run(tq, mq[0], hq[0])  # the first run sizes the buffers for the default K ...
            fq.MESSAGES_K, fq.THREADS_K = 100, 60  # ... then the instance asks for more, same shape
        r = fq.run(tq, mq[0], hq[0])
        for i in range(5):
            assert _pairs(r.terms[i]) == _single(dev, tq[i], 50, 0.85), i
        assert len(r.messages) == 100 and len(r.threads) == 60
        _check(msgs, mq[0], r.messages, 100, 0.7)
        _check(thr, hq[0], r.threads, 60, 0.7)
        assert _pairs(r.messages) == _single(mdev, mq[0], 100, 0.7) and _pairs(r.threads) == _single(hdev, hq[0], 60, 0.7)
        fq.TERMS_K = 20  # and fewer terms hits than before
        r = fq.run(tq, mq[0], hq[0])
        assert [_pairs(t) for t in r.terms] == [_single(dev, q, 20, 0.85) for q in tq]


def test_fused_bad_subset_raises_before_anything_is_enqueued():
    v, dev, seed = _terms(1294, "fp32")
    msgs, thr, mdev, hdev, mq, hq = _side()
    fq = _fused(dev)
    tq = _tq(4, seed)
    good = fq.run(tq, mq[0], hq[0])
    with pytest.raises(IndexError):
        fq.run(tq, mq[1], hq[1], message_subset=[0, 20_000])
    with pytest.raises(IndexError):
        fq.run(tq, mq[1], hq[1], message_subset=[-20_001])
    after = fq.run(tq, mq[0], hq[0])
    assert after == good


@pytest.mark.slow
def test_fused_at_a_million_rows():
    """terms and messages over 1M anisotropic fp16 rows each (bench.py's generator), T = 4 and 32: the oracle's answers"""
    import bench
    import torch

    from typeagent_py_amd.fused import FusedIndexQuery

    n = 1_000_000
    fq = FusedIndexQuery(0)
    terms = bench.gen_rows(fq.engine, 0, n, DIM, 11, "fp16", kind="aniso")
    msgs = bench.gen_rows(fq.engine, 0, n, DIM, 12, "fp16", kind="aniso")
    fq.set_corpus("terms", terms)
    fq.set_corpus("messages", msgs)
    torch.cuda.synchronize()
    tq_all = bench.aniso_queries(fq.engine, 32, DIM, 11)
    mq = bench.aniso_queries(fq.engine, 1, DIM, 12)[0]

    def chunks(t):
        for lo in range(0, n, 131_072):
            yield t[lo : lo + 131_072].float().cpu().numpy()

    positions = 0
    for T in (4, 32):
        tq = tq_all[:T]
        r = fq.run(tq, mq)
        got = [[h.item for h in hits] for hits in r.terms]
        sc, ref = vo.scores_full_chunked_refereed(chunks(terms), tq, got, 64)
        for i in range(T):
            rep, _ = vo.check_topk_parity_large(sc[i], got[i], [h.score for h in r.terms[i]], 50, 0.85, referee=ref.for_query(i))
            assert rep.k_returned == 50
            positions += rep.k_returned
        msc, mref = vo.scores_full_chunked_refereed(chunks(msgs), mq[None, :], [[h.item for h in r.messages]], 64)
        rep, _ = vo.check_topk_parity_large(msc[0], [h.item for h in r.messages], [h.score for h in r.messages], 25, 0.7, referee=mref.for_query(0))
        assert rep.k_returned == 25
        positions += rep.k_returned
    assert positions >= 2 * (4 * 50 + 25 + 10)
