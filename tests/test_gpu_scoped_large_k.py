"""GPU suite: scoped and one-mask batches beyond the fused selection -- tavb_search_scoped_topk / _device (max_hits 257 .. 16384),
tavb_search_scoped_sorted (max_hits 0 and beyond 16384) and tavb_search_subset_batch_sorted, the scoped score pass (`ScopedScoreSink`)
under `VectorBase.fuzzy_lookup_embeddings_scoped` and `fuzzy_lookup_embeddings_masked`.  The table is tests/scoped_large_k_cases.py;
tests/test_scoped_large_k_host.py pins it on the CPU.

  1. every case: the batch equals [fuzzy_lookup_embedding_masked(e, s, max_hits, thr_i)] bit for bit -- ordinals, float32 score bits,
     counts -- and passes the standing parity definition against the CPU oracle (`check_topk_parity` with the float64 referee, scores
     within SCORE_TOL); `masked_route` is 7 (257 .. 16384) or 8 (0, 16385), and what the one-mask call reports on identical handles;
  2. refinement under scopes: identical rows and tight near-duplicates, a boundary list of 64 keys, scopes that hold different halves;
  3. the score budget: "topk_scores_bytes" so small that a pass goes in sub-groups of its queries -- the answers do not change (no option
     reports the reserved size, so the check is by answers);
  4. every survivor of a scope and nothing from outside it, sorted; max_hits beyond a scope's size;
  5. the C calls: guard words, the device twin, max_total exceeded and the other argument errors;
  6. an adopted corpus with an ordinal base; a batch of more than one wave;
  7. the one-mask sorted batch equals the loop over `fuzzy_lookup_embedding_in_subset`, in one call;
  8. the scoped score pass against its numpy twin (`score_pass_twin`), one small case per tier.  The score array itself has no reader in
     the C ABI; the sorted route at k = 0 returns exactly its live slots -- a query's results ARE the positions whose slot is not "no
     score", with the slot's bits, and its count IS its histogram's sum -- so the twin is compared with that.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_large_k_cases as lc
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

E_INVALID = -1  # TAVB_E_INVALID (include/tavb.h)

_state: dict = {}


def _torch():
    import torch

    return torch


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def rows_of(corpus):
    """(the corpus' MAX_ROWS rows, the same rows as the device holds them, MAX_QUERIES queries), made once."""
    if corpus.name not in _state:
        v, _ = make_corpus(lc.MAX_ROWS, corpus.dim, corpus.seed)
        held = v.astype(np.float16).astype(np.float32) if corpus.dtype == "float16" else v
        _state[corpus.name] = (v, held, make_queries(lc.MAX_QUERIES, corpus.dim, corpus.seed + 1))
    return _state[corpus.name]


def index(corpus, rows: int):
    """The index over the first `rows` rows of the corpus, built once."""
    key = (corpus.name, rows)
    if key not in _state:
        v, held, qs = rows_of(corpus)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=corpus.dtype)
        vb.add_embeddings(None, v[:rows])
        _state[key] = (vb, held[:rows], qs)
    return _state[key]


def shared_handles(vb, scopes):
    made: dict = {}
    for s in scopes:
        if id(s) not in made:
            made[id(s)] = vb.row_mask(s)
    return [made[id(s)] for s in scopes]


def thr_of(thr, i):
    return thr[i] if isinstance(thr, list) else thr


def loop(vb, qs, handles, k, thr):
    return [vb.fuzzy_lookup_embedding_masked(qs[i], h, k, thr_of(thr, i)) for i, h in enumerate(handles)]


ORACLE_BUDGET = 20000  # hits the float64 referee judges per case before the check thins out (it takes ~0.3 ms per hit)


def assert_sorted_inside(hits, scope):
    """best first, equal scores by ascending row, and nothing from outside the scope"""
    items = np.array([h.item for h in hits], dtype=np.int64)
    scores = np.array([h.score for h in hits], dtype=np.float64)
    assert (np.lexsort((items, -scores)) == np.arange(len(hits))).all() and scope[items].all()


def check_oracle(held, qs, scopes, thr, k, got, rotate=0):
    """The standing parity check of every query's answer -- or, where the case returns more than ORACLE_BUDGET hits in all (17 queries at
    16384 hits each would take the referee half a minute), of its first and last query and one more that rotates with the case; every
    answer has been compared with the per-query call bit for bit before this."""
    nq = len(scopes)
    some = range(nq) if sum(len(x) for x in got) <= ORACLE_BUDGET else sorted({0, nq - 1, rotate % nq})
    for i in some:
        scope = scopes[i]
        flat = np.flatnonzero(scope)
        if len(flat) == 0:
            assert got[i] == []
            continue
        t = thr_of(thr, i)
        sub = held[flat]
        vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [h.item for h in got[i]], [h.score for h in got[i]], k if k else len(flat),
                             0.0 if t is None else t, candidate_ordinals=flat, referee=vo.f64_referee(sub, qs[i]))


# ---- 1. every case through the class -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lc.CASES, ids=[c.name for c in lc.CASES])
def test_case(case):
    vb, held, qs = index(case.corpus, case.rows)
    eng = vb.engine
    scopes = lc.case_scopes(case)
    thr = lc.case_thresholds(case)
    handles = shared_handles(vb, scopes)
    want = loop(vb, qs, handles, case.max_hits, thr)
    native = lc.expect_native(scopes)
    one_mask = None
    if not native and len({id(s) for s in scopes}) == 1 and scopes[0].any():
        vb.fuzzy_lookup_embeddings_masked(qs[: case.nq], handles[0], case.max_hits, thr)
        one_mask = eng.get_option("masked_route")
    if native:  # a one-scope lookup first, so that the 7 or 8 below is this call's
        vb.fuzzy_lookup_embeddings_masked(qs[:1], np.ones(case.rows, dtype=bool), 1)
        assert eng.get_option("masked_route") == 1
    before = eng.get_option("masked_route")
    got = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles if case.as_handles else scopes, case.max_hits, thr)
    assert len(got) == case.nq
    if native:
        assert eng.get_option("masked_route") == lc.route_of(case.max_hits)
        assert eng.get_option("last_tier") == case.corpus.tier
    elif one_mask is not None:
        assert eng.get_option("masked_route") == one_mask == 1  # one scope for all: the one-mask call, on the row list
    else:
        assert eng.get_option("masked_route") == before and got == [[] for _ in range(case.nq)]  # nothing to search: no call
    assert [bits32(x) for x in got] == [bits32(x) for x in want], case.name
    for i, scope in enumerate(scopes):
        assert_sorted_inside(got[i], scope)
    check_oracle(held, qs, scopes, thr, case.max_hits, got, rotate=case.seed)


# ---- 2. refinement under scopes --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["identical_rows", "near_duplicates"])
def test_refinement_under_scopes(kind):
    n, d, k = 6000, 72, 300
    v, _ = make_corpus(n, d, 9990)
    qs = make_queries(4, d, 9991)
    dup = np.arange(1000, 5000)  # 4000 rows that are one row, or that row plus noise of a few float32 ulps
    v[dup] = v[1000]
    if kind == "near_duplicates":
        v[dup] += np.random.default_rng(9992).normal(0, 2e-7, (len(dup), d)).astype(np.float32)
    qs[:] = v[1000] + 0.05 * qs  # the duplicates are every query's best rows
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    vb.add_embeddings(None, v)
    eng = vb.engine
    scopes = []
    for j in range(4):  # each scope a different half of the duplicates, plus every other row
        s = np.ones(n, dtype=bool)
        s[dup[(np.arange(len(dup)) + j) % 4 >= 2]] = False
        scopes.append(s)
    handles = [vb.row_mask(s) for s in scopes]
    want = loop(vb, qs, handles, k, 0.0)
    eng.set_option("topk_boundary_keys", 64)
    try:
        got = vb.fuzzy_lookup_embeddings_scoped(qs, handles, k, 0.0)
        assert eng.get_option("masked_route") == 7 and eng.get_option("last_topk_refine") >= 1
        again = loop(vb, qs, handles, k, 0.0)
    finally:
        eng.set_option("topk_boundary_keys", 16384)
    assert [bits32(x) for x in got] == [bits32(x) for x in want] == [bits32(x) for x in again]
    for i in range(4):
        assert len(got[i]) == k and all(scopes[i][h.item] for h in got[i])
        if kind == "identical_rows":  # one score for all 300: the first 300 duplicates the scope holds, ascending
            assert [h.item for h in got[i]] == [r for r in dup if scopes[i][r]][:k]


# ---- 3. the score budget ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_hits", [300, 0, 16385])
def test_score_budget_cuts_a_pass_into_sub_groups(max_hits):
    case = lc.Case(lc.CORPORA[3], 4099, 17, max_hits, "random50%", "per_query", True)
    vb, held, qs = index(case.corpus, case.rows)
    eng = vb.engine
    scopes = lc.case_scopes(case)
    thr = lc.case_thresholds(case)
    handles = shared_handles(vb, scopes)
    want = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles, max_hits, thr)
    # the union of eight 50 % scopes is nearly every row: 3 x 4099 x 4 bytes hold three queries of a pass, so a pass of eight goes as 3 + 3 + 2
    eng.set_option("topk_scores_bytes", 3 * 4099 * 4)
    try:
        got = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles, max_hits, thr)
        assert eng.get_option("masked_route") == lc.route_of(max_hits) and eng.get_option("topk_scores_bytes") == 3 * 4099 * 4
        one = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles, max_hits, thr) if eng.set_option("topk_scores_bytes", 4096) is None else None
    finally:
        eng.set_option("topk_scores_bytes", 1 << 30)
    assert [bits32(x) for x in got] == [bits32(x) for x in want] == [bits32(x) for x in one]  # (4096 bytes: one query per sub-group)
    assert [bits32(x) for x in want] == [bits32(x) for x in loop(vb, qs, handles, max_hits, thr)]


# ---- 4. every survivor of a scope ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_hits", [0, 5000, 16385])
def test_every_survivor_of_the_scope_and_nothing_else(max_hits):
    corpus = lc.CORPORA[0]
    vb, held, qs = index(corpus, 4099)
    rng = np.random.default_rng(9993)
    scopes = [rng.random(4099) < p for p in (0.5, 0.05, 0.9)]  # 5000 and 16385 exceed every scope
    thr = [0.0, 0.5, 0.52]
    got = vb.fuzzy_lookup_embeddings_scoped(qs[:3], scopes, max_hits, thr)
    assert vb.engine.get_option("masked_route") == lc.route_of(max_hits)  # (5000: the large-k route with k beyond every scope)
    for i, scope in enumerate(scopes):
        sc = vo.cosine_to_score(np.dot(held, qs[i]))
        survivors = np.flatnonzero(scope & (sc >= np.float32(thr[i])))
        near = np.flatnonzero(scope & (np.abs(sc - np.float32(thr[i])) < 1e-6))  # rows whose float32 score may fall on either side
        assert set(survivors) - set(near) <= {h.item for h in got[i]} <= set(survivors) | set(near)
        assert_sorted_inside(got[i], scope)


# ---- 5. the C calls --------------------------------------------------------------------------------------------------------------------------

def _c_case():
    case = lc.Case(lc.CORPORA[3], 1000, 9, 300, "nested", "per_query", True)
    vb, held, qs = index(case.corpus, case.rows)
    scopes = lc.case_scopes(case)
    handles = shared_handles(vb, scopes)
    thr = lc.case_thresholds(case)
    t = np.asarray([_native.f32_threshold(0.0 if x is None else x) for x in thr], dtype=np.float32)
    return case, vb, np.ascontiguousarray(qs[: case.nq]), handles, thr, t


def test_guard_words_and_the_device_twin():
    torch = _torch()
    case, vb, q, handles, thr, t = _c_case()
    eng = vb.engine
    nq, k = case.nq, case.max_hits
    want = loop(vb, q, handles, k, thr)
    bits = [h.dev_bits for h in handles]
    ptrs = (ctypes.c_void_p * nq)(*[b.data_ptr() for b in bits])
    a = _native._addr
    ords, scs, cnts = np.full(nq * k + 1, -77, dtype=np.int64), np.full(nq * k + 1, -77.0, dtype=np.float32), np.full(nq + 1, -77, dtype=np.int32)
    rc = eng.lib.tavb_search_scoped_topk(eng._h, a(q), nq, ptrs, case.rows, k, a(t), a(ords), a(scs), a(cnts))
    assert rc == 0, eng.lib.tavb_last_error()
    assert ords[-1] == -77 and scs[-1] == -77.0 and cnts[-1] == -77, "an element behind an output buffer was written"
    assert eng.get_option("masked_route") == 7
    o2, s2 = ords[:-1].reshape(nq, k), scs[:-1].reshape(nq, k)
    for i in range(nq):
        assert list(zip(o2[i, : cnts[i]].tolist(), s2[i, : cnts[i]].view(np.uint32).tolist())) == bits32(want[i]), i
    # the device twin: keys behind which one more key stays untouched, equal to the synchronous call's
    out = torch.full((nq * k + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_scoped_topk_device(torch.from_numpy(q).cuda(), bits, k, t, out_keys=out)
    eng.synchronize()
    keys = out.cpu().numpy()
    assert keys[-1] == 0x5A5A5A5A5A5A5A5A, "the key behind the device twin's output was written"
    keys = keys[:-1].view(np.uint64).reshape(nq, k)
    for i in range(nq):
        live = keys[i][keys[i] != 0]
        assert len(live) == cnts[i] and (keys[i][len(live):] == 0).all()
        assert list(zip((0xFFFFFFFF - (live & np.uint64(0xFFFFFFFF))).astype(np.int64).tolist(), (live >> np.uint64(32)).astype(np.uint32).tolist())) == bits32(want[i])
    # the sorted call: the concatenated outputs with a word behind them, counts and total
    want0 = loop(vb, q, handles, 0, thr)
    total_want = sum(len(x) for x in want0)
    ords, scs, c64 = np.full(total_want + 1, -77, dtype=np.int64), np.full(total_want + 1, -77.0, dtype=np.float32), np.full(nq + 1, -77, dtype=np.int64)
    total = ctypes.c_int64(-1)
    rc = eng.lib.tavb_search_scoped_sorted(eng._h, a(q), nq, ptrs, case.rows, 0, a(t), total_want, a(ords), a(scs), a(c64), ctypes.byref(total))
    assert rc == 0, eng.lib.tavb_last_error()
    assert total.value == total_want and c64[:-1].tolist() == [len(x) for x in want0] and eng.get_option("masked_route") == 8
    assert ords[-1] == -77 and scs[-1] == -77.0 and c64[-1] == -77
    assert list(zip(ords[:-1].tolist(), scs[:-1].view(np.uint32).tolist())) == [p for x in want0 for p in bits32(x)]
    # one result too many for max_total
    rc = eng.lib.tavb_search_scoped_sorted(eng._h, a(q), nq, ptrs, case.rows, 0, a(t), total_want - 1, a(ords), a(scs), a(c64), ctypes.byref(total))
    assert rc == E_INVALID and b"max_total" in eng.lib.tavb_last_error()


def test_argument_errors():
    case, vb, q, handles, thr, t = _c_case()
    eng = vb.engine
    nq, k, rows = case.nq, case.max_hits, case.rows
    bits = [h.dev_bits for h in handles]
    ptrs = (ctypes.c_void_p * nq)(*[b.data_ptr() for b in bits])
    holed = (ctypes.c_void_p * nq)(*[None if i == 4 else b.data_ptr() for i, b in enumerate(bits)])
    a = _native._addr
    ords, scs, cnts, c64 = np.zeros(nq * k, np.int64), np.zeros(nq * k, np.float32), np.zeros(nq, np.int32), np.zeros(nq, np.int64)
    total = ctypes.c_int64(0)
    lib, h = eng.lib, eng._h
    inv = E_INVALID

    def topk(**kw):
        p = dict(q=a(q), nq=nq, masks=ptrs, rows=rows, k=k, t=a(t), o=a(ords), s=a(scs), c=a(cnts))
        p.update(kw)
        return lib.tavb_search_scoped_topk(h, p["q"], p["nq"], p["masks"], p["rows"], p["k"], p["t"], p["o"], p["s"], p["c"])

    def srt(**kw):
        p = dict(q=a(q), nq=nq, masks=ptrs, rows=rows, k=0, t=a(t), mt=nq * k, o=a(ords), s=a(scs), c=a(c64), tot=ctypes.byref(total))
        p.update(kw)
        return lib.tavb_search_scoped_sorted(h, p["q"], p["nq"], p["masks"], p["rows"], p["k"], p["t"], p["mt"], p["o"], p["s"], p["c"], p["tot"])

    for bad, word in ((dict(q=None), b"null"), (dict(t=None), b"null"), (dict(o=None), b"null"), (dict(c=None), b"null"), (dict(masks=None), b"null dev_masks"),
                      (dict(masks=holed), b"query 4 is null"), (dict(rows=rows + 1), b"the corpus has"), (dict(k=0), b"k must be"),
                      (dict(k=16385), b"1 <= k <= 16384"), (dict(nq=-1), b"nq must be")):
        assert topk(**bad) == inv and word in lib.tavb_last_error(), bad
    for bad, word in ((dict(q=None), b"null"), (dict(c=None), b"null"), (dict(tot=None), b"null"), (dict(masks=holed), b"query 4 is null"),
                      (dict(rows=rows - 1), b"the corpus has"), (dict(k=-1), b"k must be"), (dict(mt=-1), b"max_total"), (dict(o=None), b"null")):
        assert srt(**bad) == inv and word in lib.tavb_last_error(), bad
    out = _torch().zeros((nq, k), dtype=_torch().int64, device="cuda")
    assert lib.tavb_search_scoped_topk_device(h, None, nq, ptrs, rows, k, a(t), ctypes.c_void_p(out.data_ptr())) == inv
    assert lib.tavb_search_scoped_topk_device(h, ctypes.c_void_p(out.data_ptr()), nq, holed, rows, k, a(t), ctypes.c_void_p(out.data_ptr())) == inv
    dev_rows = handles[-1].dev_rows
    rp, n = ctypes.c_void_p(dev_rows.data_ptr()), int(dev_rows.numel())
    assert lib.tavb_search_subset_batch_sorted(h, a(q), nq, None, n, 0, a(t), nq * n, a(ords), a(scs), a(c64), ctypes.byref(total)) == inv
    assert lib.tavb_search_subset_batch_sorted(h, a(q), nq, rp, -1, 0, a(t), nq * n, a(ords), a(scs), a(c64), ctypes.byref(total)) == inv
    assert lib.tavb_search_subset_batch_sorted(h, a(q), nq, rp, n, -1, a(t), nq * n, a(ords), a(scs), a(c64), ctypes.byref(total)) == inv
    assert lib.tavb_search_subset_batch_sorted(h, a(q), nq, rp, n, 0, a(t), 1, a(ords), a(scs), a(c64), ctypes.byref(total)) == inv
    assert b"max_total" in lib.tavb_last_error()
    assert topk(nq=0) == 0 and srt(nq=0) == 0 and total.value == 0  # no query: nothing to do
    assert topk() == 0, lib.tavb_last_error()  # ... and the context still serves


# ---- 6. an adopted corpus; more than one wave ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", lc.ADOPTED, ids=[c.name for c in lc.ADOPTED])
def test_adopted_corpus_with_an_ordinal_base(case):
    torch = _torch()
    _, held, qs = rows_of(case.corpus)
    held = held[: case.rows]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    vb.adopt_device_corpus(torch.from_numpy(held.astype(np.float16)).cuda(), ordinal_base=lc.ORDINAL_BASE)
    eng = vb.engine
    assert eng.ordinal_base == lc.ORDINAL_BASE
    scopes = lc.case_scopes(case)
    thr = lc.case_thresholds(case)
    handles = shared_handles(vb, scopes)
    got = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles, case.max_hits, thr)
    assert eng.get_option("masked_route") == lc.route_of(case.max_hits)
    assert [bits32(x) for x in got] == [bits32(x) for x in loop(vb, qs, handles, case.max_hits, thr)]
    check_oracle(held, qs, scopes, thr, case.max_hits, got)
    # the engine's own ordinals carry the base
    t = np.asarray([_native.f32_threshold(0.0 if x is None else x) for x in thr], dtype=np.float32)
    bits = [h.dev_bits for h in handles]
    if case.max_hits:
        o, s, c = eng.search_scoped_topk(qs[: case.nq], bits, case.max_hits, t)
        flat = [o[i, : c[i]] for i in range(case.nq)]
    else:
        o, s, c = eng.search_scoped_sorted(qs[: case.nq], bits, 0, t, sum(h.count for h in handles))
        flat = np.split(o, np.cumsum(c)[:-1])
    for i in range(case.nq):
        assert (flat[i] - lc.ORDINAL_BASE).tolist() == [h.item for h in got[i]]


@pytest.mark.parametrize("max_hits", [300, 0])
def test_a_batch_of_more_than_one_wave(max_hits):
    corpus = lc.CORPORA[0]
    vb, held, _ = index(corpus, 1000)
    nq = 131  # 16 passes of eight are a wave: 128 + 3
    qs = make_queries(nq, corpus.dim, 9994)
    rng = np.random.default_rng(9995)
    pool = [rng.random(1000) < p for p in (0.5, 0.3, 0.02, 0.9, 0.0)]
    scopes = [pool[(i * 7) % 5] for i in range(nq)]
    thr = [lc.THR_CYCLE[i % len(lc.THR_CYCLE)] for i in range(nq)]
    handles = shared_handles(vb, scopes)
    got = vb.fuzzy_lookup_embeddings_scoped(qs, handles, max_hits, thr)
    assert vb.engine.get_option("masked_route") == lc.route_of(max_hits)
    assert [bits32(x) for x in got] == [bits32(x) for x in loop(vb, qs, handles, max_hits, thr)]


# ---- 7. the one-mask sorted batch ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus", [lc.CORPORA[1], lc.CORPORA[4]], ids=lambda c: c.name)
@pytest.mark.parametrize("max_hits", [0, 16385])
def test_one_mask_sorted_batch_equals_the_subset_loop(corpus, max_hits, monkeypatch):
    vb, held, qs = index(corpus, 20000)
    eng = vb.engine
    scope = np.random.default_rng(9996).random(20000) < 0.9  # 18000 rows: more than 16385
    h = vb.row_mask(scope)
    flat = np.flatnonzero(scope)
    thr = [lc.THR_CYCLE[i % len(lc.THR_CYCLE)] for i in range(9)]
    calls = []
    real = eng.search_subset_batch_sorted
    monkeypatch.setattr(eng, "search_subset_batch_sorted", lambda *a, **kw: calls.append(len(a[0])) or real(*a, **kw))
    got = vb.fuzzy_lookup_embeddings_masked(qs[:9], h, max_hits, thr)
    assert calls == [9] and eng.get_option("masked_route") == 1  # ONE call for the nine queries, on the row list
    want = [vb.fuzzy_lookup_embedding_in_subset(qs[i], flat, max_hits, thr[i]) for i in range(9)]
    assert calls == [9]  # (the subset lookups are the single-query call's)
    assert [bits32(x) for x in got] == [bits32(x) for x in want]
    assert len(got[0]) == (len(flat) if max_hits == 0 else 16385) and got[4] == []


# ---- 8. the scoped score pass against its numpy twin -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus", [lc.CORPORA[0], lc.CORPORA[1], lc.CORPORA[2], lc.CORPORA[5]], ids=lambda c: c.name)
def test_scoped_score_pass_equals_the_numpy_twin(corpus):
    rows = 1000
    vb, held, qs = index(corpus, rows)
    eng = vb.engine
    rng = np.random.default_rng(9997)
    masks = [rng.random(rows) < p for p in (0.5, 0.1, 0.9, 0.5, 0.02, 0.5, 0.7, 0.3)]
    masks[4][:] = False  # an empty scope inside the pass
    union = np.flatnonzero(np.logical_or.reduce(masks))
    member = lc.member_bytes(masks, union)
    thr = np.asarray([0.0, 0.5, 0.45, 0.55, 0.0, 0.4, 1.5, 0.5], dtype=np.float32)
    # the single-query pass' score of every union position: the sorted lookup of that query alone over the union list, threshold 0
    single = np.zeros((8, len(union)), dtype=np.float32)
    for j in range(8):
        pos, scs = eng.search_subset_sorted(qs[j], union, 0, np.float32(0.0))
        single[j, pos] = scs
        assert len(pos) == len(union)  # (scores of unit rows and queries: none below 0)
    want, counts = lc.score_pass_twin(single, member, thr)
    handles = [vb.row_mask(m) for m in masks]
    o, s, c = eng.search_scoped_sorted(qs[:8], [h.dev_bits for h in handles], 0, thr, int(sum(m.sum() for m in masks)))
    assert eng.get_option("masked_route") == 8 and eng.get_option("last_tier") == corpus.tier
    assert c.tolist() == counts  # the histograms' sums: members that pass
    got = np.full((8, len(union)), lc.SCORE_NONE, dtype=np.uint32)
    at = np.concatenate([[0], np.cumsum(c)])
    for j in range(8):
        got[j, np.searchsorted(union, o[at[j]: at[j + 1]])] = s[at[j]: at[j + 1]].view(np.uint32)
    np.testing.assert_array_equal(got, want)
