"""GPU suite: exact top-k beyond the fused selection (TAVB_MAX_FUSED_K < k <= TAVB_MAX_LARGE_K: tavb_search_topk /
tavb_search_subset_topk, csrc/tavb_topk.hip) -- the score pass against the streaming scan bit for bit, the answers against the
emit-all route and the oracle, the boundary refinement on degenerate score distributions, the batched class call and the switch."""

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.fakes import NullModel
from tests.synth import make_clustered_corpus, make_corpus, make_queries, subset_choice
from typeagent_py_amd import ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

MAX_K = _native.MAX_LARGE_K


def new_vb(vectors, dtype="fp32") -> VectorBase:
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    vb.add_embeddings(None, np.ascontiguousarray(vectors, dtype=np.float32))
    return vb


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def items_scores(res):
    assert all(isinstance(r, ScoredInt) for r in res)
    return [r.item for r in res], [r.score for r in res]


def assert_same(a, b):
    """(ordinals, scores) pairs equal bit for bit"""
    np.testing.assert_array_equal(np.asarray(a[0]), np.asarray(b[0]))
    np.testing.assert_array_equal(np.asarray(a[1], dtype=np.float32).view(np.uint32), np.asarray(b[1], dtype=np.float32).view(np.uint32))


def special_rows(v):
    v = v.copy()
    v[5] = np.nan
    v[11] = np.inf
    v[17] = -np.inf
    v[23] = 0.0
    v[29, 0] = np.nan
    return v


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [3, 100, 384, 1536, 3072])
def test_score_pass_is_the_streaming_scan(dtype, d):
    """k <= 256: every query's row of search_topk equals that query's fused lookup (the streaming scan) bit for bit -- ordinals, score
    bits, counts -- across the three scan tiers, batches cut into groups of 8, per-query thresholds and NaN / inf / zero rows."""
    n = 2500
    v, _ = make_corpus(n, d, 9100 + d)
    v = special_rows(v)
    vb = new_vb(v, dtype)
    eng = vb.engine
    qs = make_queries(20, d, 9200 + d)
    qs[4] = v[40]  # a query equal to a row
    thr_cycle = np.array([0.0, 0.5, 1.0, 1.5, -0.2, 0.45, 0.55, 0.0], dtype=np.float32)
    for nq in (1, 3, 8, 9, 20):
        thrs = thr_cycle[np.arange(nq) % len(thr_cycle)]
        for k in (1, 10, 64, 256):
            ords, scs, cnts = eng.search_topk(qs[:nq], k, thrs)
            for i in range(nq):
                o1, s1 = eng.search(qs[i], k, thrs[i])
                assert cnts[i] == len(o1), (nq, k, i)
                assert_same((ords[i, : cnts[i]], scs[i, : cnts[i]]), (o1, s1))


@pytest.mark.parametrize("dtype,n,d", [("fp32", 20_000, 384), ("fp16", 30_000, 1536), ("fp32", 5_000, 100)])
def test_large_k_equals_emit_all_and_oracle(dtype, n, d):
    """K in {257, 1000, 4096, MAX_LARGE_K}: the emit-all route's answer (tavb_search_all, sorted on the host) bit for bit, and the oracle's
    modulo fp32 near-ties; fewer survivors than K, K beyond the rows."""
    v, q = make_corpus(n, d, 9300 + d)
    vb = new_vb(v, dtype)
    eng = vb.engine
    vv = _f16(v) if dtype == "fp16" else v
    sc = vo.scores_full(vv, q)
    high = float(np.sort(sc)[-700])  # ~700 survivors: fewer than most K below
    for thr in (np.float32(0.0), np.float32(high)):
        for k in (257, 1000, 4096, MAX_K):
            ords, scs, cnts = eng.search_topk(q[None], k, thr)
            m = int(cnts[0])
            want = eng.search_all(q, thr, k)
            assert_same((ords[0, :m], scs[0, :m]), want)
            vo.check_topk_parity(sc, ords[0, :m].tolist(), scs[0, :m].tolist(), k, float(thr), referee=vo.f64_referee(vv, q))
    assert eng.get_option("last_topk_refine") == 0


def test_subset_through_the_class_against_the_old_route():
    """fuzzy_lookup_embedding_in_subset with max_hits > 256 (negative and duplicate ordinals, numpy index semantics) equals the
    emit-all route (large_k = 0) bit for bit."""
    n, d = 12_000, 384
    v, q = make_corpus(n, d, 9400)
    vb = new_vb(v)
    sub = subset_choice(n, 6000, 9401) + [0, 0, -1, -n, 17, 17, 17]
    res = {}
    for large in (1, 0):
        vb.engine.set_option("large_k", large)
        for k in (257, 1000, 5000, 7000):
            for ms in (0.0, 0.52):
                res[(large, k, ms)] = vb.fuzzy_lookup_embedding_in_subset(q, sub, max_hits=k, min_score=ms)
    vb.engine.set_option("large_k", 1)
    for k in (257, 1000, 5000, 7000):
        for ms in (0.0, 0.52):
            assert_same(items_scores(res[(1, k, ms)]), items_scores(res[(0, k, ms)]))


@pytest.mark.parametrize("k", [300, 4096])
def test_identical_rows_refine_to_ascending_ordinals(k):
    """5000 identical rows in one bucket: the answer is ordinals 0 .. K-1; with a boundary list smaller than 5000 the bucket is refined
    (last_topk_refine >= 1) and the answer is the same."""
    d = 384
    row = make_queries(1, d, 9500)[0]
    v = np.repeat(row[None], 5000, axis=0)
    vb = new_vb(v)
    eng = vb.engine
    q = make_queries(1, d, 9501)[0] * 0.3 + row
    q /= np.linalg.norm(q)
    ords, scs, cnts = eng.search_topk(q[None], k, np.float32(0.0))
    assert cnts[0] == k and ords[0].tolist() == list(range(k))
    assert len(set(scs[0].tolist())) == 1
    assert eng.get_option("last_topk_refine") == 0
    for cap in (1024, 64):
        eng.set_option("topk_boundary_keys", cap)
        o2, s2, c2 = eng.search_topk(q[None], k, np.float32(0.0))
        assert eng.get_option("last_topk_refine") >= 1
        assert_same((o2, s2), (ords, scs))
        assert c2[0] == k
    res = vb.fuzzy_lookup_embedding(q, max_hits=k, min_score=0.0)
    assert [r.item for r in res] == list(range(k))


def test_clustered_near_duplicates_refine():
    """Clusters of 3000 near-duplicates (an eighth of them exact duplicates): the queries' boundary buckets hold thousands of keys;
    with small boundary lists they are refined, and the answers equal the emit-all route's and the oracle's."""
    v, qs, _, _ = make_clustered_corpus(30_000, 384, 9600, cluster_rows=3000, n_queries=6)
    vb = new_vb(v)
    eng = vb.engine
    ref = {}
    for i, q in enumerate(qs):
        for k in (1000, 4096):
            ref[(i, k)] = eng.search_all(q, np.float32(0.0), k)
    for cap in (16384, 512):
        eng.set_option("topk_boundary_keys", cap)
        for k in (1000, 4096):
            ords, scs, cnts = eng.search_topk(qs, k, np.float32(0.0))
            if cap == 512:
                assert eng.get_option("last_topk_refine") >= 1
            for i in range(len(qs)):
                assert_same((ords[i, : cnts[i]], scs[i, : cnts[i]]), ref[(i, k)])
    for i, q in enumerate(qs[:2]):
        ords, scs = ref[(i, 1000)]
        vo.check_topk_parity(vo.scores_full(v, q), ords.tolist(), scs.tolist(), 1000, 0.0, referee=vo.f64_referee(v, q))


def test_anisotropic_rows_high_threshold():
    """Rows packed around one direction (every score near 0.9) at min_score 0.85: one narrow band of buckets over [0.85, 1]."""
    n, d = 40_000, 384
    rng = np.random.default_rng(9700)
    axis = rng.standard_normal(d).astype(np.float32)
    axis /= np.linalg.norm(axis)
    v = axis[None] + np.float32(0.35) * rng.standard_normal((n, d)).astype(np.float32) / np.float32(np.sqrt(d))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    q = axis + np.float32(0.05) * rng.standard_normal(d).astype(np.float32) / np.float32(np.sqrt(d))
    q /= np.linalg.norm(q)
    vb = new_vb(v)
    eng = vb.engine
    sc = vo.scores_full(v, q)
    assert np.sum(sc >= np.float32(0.85)) > 10_000
    for cap in (16384, 256):
        eng.set_option("topk_boundary_keys", cap)
        for k in (1000, 4096, MAX_K):
            ords, scs, cnts = eng.search_topk(q[None], k, np.float32(0.85))
            m = int(cnts[0])
            assert_same((ords[0, :m], scs[0, :m]), eng.search_all(q, np.float32(0.85), k))
        if cap == 256:
            assert eng.get_option("last_topk_refine") >= 1
    vo.check_topk_parity(sc, ords[0, :m].tolist(), scs[0, :m].tolist(), MAX_K, 0.85, referee=vo.f64_referee(v, q))


def test_batched_class_call_is_one_call():
    """fuzzy_lookup_embeddings(qs[40], max_hits=1000) equals the 40 single lookups, in ceil(40 / 8) = 5 corpus passes (the per-query
    loop made 40 emit-all passes); per-query thresholds are honoured."""
    n, d = 50_000, 1536
    v, _ = make_corpus(n, d, 9800)
    vb = new_vb(v, "fp16")
    qs = make_queries(40, d, 9801)
    eng = vb.engine
    eng.profile_enable(True)
    eng.profile_reset()
    batch = vb.fuzzy_lookup_embeddings(qs, max_hits=1000, min_score=0.0)
    assert eng.profile_read(_native.KERNEL_SCAN)[1] <= 5
    assert eng.profile_read(_native.KERNEL_TOPK)[1] >= 1
    eng.profile_enable(False)
    for i, q in enumerate(qs):
        assert_same(items_scores(batch[i]), items_scores(vb.fuzzy_lookup_embedding(q, max_hits=1000, min_score=0.0)))
    thrs = [0.0, 0.5, 0.51, None] * 10
    mixed = vb.fuzzy_lookup_embeddings(qs, max_hits=700, min_score=thrs)
    for i, q in enumerate(qs):
        assert_same(items_scores(mixed[i]), items_scores(vb.fuzzy_lookup_embedding(q, max_hits=700, min_score=thrs[i])))


def test_switch_restores_the_emit_all_route():
    n, d = 8000, 384
    v, q = make_corpus(n, d, 9900)
    vb = new_vb(v)
    eng = vb.engine
    assert eng.get_option("large_k") == 1
    eng.profile_enable(True)
    out = {}
    for large in (1, 0):
        eng.set_option("large_k", large)
        eng.profile_reset()
        out[large] = vb.fuzzy_lookup_embedding(q, max_hits=2000, min_score=0.1)
        assert eng.profile_read(_native.KERNEL_TOPK)[1] == large
        out[(large, "b")] = vb.fuzzy_lookup_embeddings(np.stack([q, q * 0.5]), max_hits=300, min_score=0.0)
    eng.profile_enable(False)
    eng.set_option("large_k", 1)
    assert_same(items_scores(out[1]), items_scores(out[0]))
    for a, b in zip(out[(1, "b")], out[(0, "b")]):
        assert_same(items_scores(a), items_scores(b))
    # unchanged routes: max_hits == 0 (all survivors) and max_hits beyond MAX_LARGE_K
    assert len(vb.fuzzy_lookup_embedding(q, max_hits=0, min_score=0.0)) == n
    assert len(vb.fuzzy_lookup_embedding(q, max_hits=MAX_K + 1, min_score=0.0)) == n
    with pytest.raises(ValueError, match="k must be"):
        eng.search_topk(q[None], MAX_K + 1, np.float32(0.0))
    with pytest.raises(ValueError, match="topk_boundary_keys"):
        eng.set_option("topk_boundary_keys", 10)


def test_small_score_budget_cuts_the_groups():
    """topk_scores_bytes below 8 queries' score arrays: more, smaller corpus passes, the same answers."""
    n, d = 20_000, 384
    v, _ = make_corpus(n, d, 9950)
    vb = new_vb(v)
    eng = vb.engine
    qs = make_queries(11, d, 9951)
    want = eng.search_topk(qs, 500, np.float32(0.0))
    eng.set_option("topk_scores_bytes", 3 * n * 4)
    eng.profile_enable(True)
    eng.profile_reset()
    got = eng.search_topk(qs, 500, np.float32(0.0))
    assert eng.profile_read(_native.KERNEL_SCAN)[1] == 4  # groups of 3
    eng.profile_enable(False)
    for a, b in zip(want, got):
        np.testing.assert_array_equal(a, b)


@pytest.mark.slow
def test_two_million_rows_k4096_against_chunked_oracle():
    """2M x 1536 fp16, 16 queries, K = 4096 in two corpus passes, checked against the oracle over the whole corpus."""
    from bench import ORACLE_CHUNK, host_queries, make_device_corpus

    rows, dim, nq, k = 2_000_000, 1536, 16, 4096
    eng = _native.Engine(0)
    corpus = make_device_corpus(eng, rows, dim, 12_345, "fp16")
    eng.set_corpus_tensor(corpus)
    qs = host_queries(nq, dim, 777)
    qs[3] = corpus[1_234_567].float().cpu().numpy()
    ords, scs, cnts = eng.search_topk(qs, k, np.float32(0.0))
    assert np.all(cnts == k) and np.all(np.diff(scs, axis=1) <= 0)
    assert ords[3, 0] == 1_234_567
    for i in (0, 3):
        o1, s1 = eng.search_all(qs[i], np.float32(0.0), k)
        assert_same((ords[i], scs[i]), (o1, s1))
    ref = vo.scores_full_chunked((corpus[lo : lo + ORACLE_CHUNK].float().cpu().numpy() for lo in range(0, rows, ORACLE_CHUNK)), qs)
    for i in range(nq):
        vo.check_topk_parity_large(ref[i], ords[i].tolist(), scs[i].tolist(), k, 0.0)
    eng.close()
