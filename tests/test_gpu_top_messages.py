"""GPU suite: top-k distinct messages on the device -- `MessageMaxSink` and `message_hist_kernel` behind tavb_search_top_messages /
_device, under `VectorBase.lookup_top_messages_by_embedding(s)` and `adapters.lookup_top_messages`.  The table is
tests/top_messages_cases.py; tests/test_top_messages_host.py pins it on the CPU.

  1. every case against expected answer A -- the library's own exact row scores: `fuzzy_lookup_embedding(e, max_hits=len(vb),
     min_score=t)` (`_masked` with the same mask), collapsed in numpy by max per message, sorted by (-score, message), cut at K -- in
     ordinals, float32 score bits and counts; the batch equals the loop of single calls and `top_messages` = 0 (the host collapse) equals
     the native route, both bit for bit;
  2. one case per corpus against expected answer B, the reference's arithmetic (`top_messages_cases.judge_b`);
  3. the tie case: 600 equal rows in 600 messages, K = 100, a boundary list of 64 keys -- ordinal order, and the refinement rounds ran;
  4. tavb_search_top_messages_device equals the host-query form, also with n_messages beyond every ordinal in use;
  5. after `insert_rows(..., row_messages=...)` and after `remove_rows` the answer is a fresh index's over numpy's result;
  6. errors and fallbacks: no map, a map that does not cover the corpus, K = 0 and K = 16385, a stale `RowMask`;
  7. the lookup this call exists for: 40 messages x 8 chunks, `lookup_messages_by_embedding(e, 5)` returns fewer than 5 messages,
     `lookup_top_messages_by_embedding(e, 5)` returns 5 with the same first entry."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import top_messages_cases as tc
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

pytestmark = pytest.mark.gpu

_state: dict = {}


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def make_index(v, dtype, rm=None):
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    if rm is not None:
        vb.set_row_messages(rm)
    return vb


def index(corpus: tc.Corpus):
    """One VectorBase per corpus, built once; the case sets its map."""
    if corpus not in _state:
        _state[corpus] = make_index(tc.corpus_arrays(corpus)[0], corpus.dtype)
    return _state[corpus]


def row_hits(vb, case, qi, handle):
    """Expected answer A's input: every passing row of query qi with the library's own exact scores, once per (corpus, query, threshold, mask)."""
    thr = tc.threshold_of(case, qi)
    key = ("rows", case.corpus, qi, thr, case.allowed, case.map if case.allowed == "message_mask" else None)
    if key not in _state:
        q = tc.corpus_arrays(case.corpus)[2][qi]
        n = len(vb)
        hits = vb.fuzzy_lookup_embedding(q, max_hits=n, min_score=thr) if handle is None else vb.fuzzy_lookup_embedding_masked(q, handle, n, thr)
        _state[key] = ([h.item for h in hits], [h.score for h in hits])
    return _state[key]


def answer_a(vb, case, qi, handle):
    rows, scores = row_hits(vb, case, qi, handle)
    m, s = tc.collapse(rows, scores, tc.message_map(case.corpus.rows, case.map), tc.case_k(case))
    return list(zip(m.tolist(), s.view(np.uint32).tolist()))


def case_handle(vb, case):
    mask = tc.case_mask(case)
    if mask is None:
        return None
    return vb.message_mask(tc.allowed_messages(case)) if case.allowed == "message_mask" else vb.row_mask(mask)


# ---- 1. every case against A ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_case_against_the_librarys_own_scores(case):
    vb = index(case.corpus)
    vb.set_row_messages(tc.message_map(case.corpus.rows, case.map))
    qs = tc.corpus_arrays(case.corpus)[2][: case.nq]
    handle = case_handle(vb, case)
    k, thr = tc.case_k(case), tc.case_thresholds(case)
    eng = vb.engine
    assert eng.get_option("top_messages") == 1
    got = vb.lookup_top_messages_by_embeddings(qs, k, thr, handle)
    assert len(got) == case.nq
    for qi in range(case.nq):
        want = answer_a(vb, case, qi, handle)
        assert bits32(got[qi]) == want, f"{case.name} q{qi}: {bits32(got[qi])[:5]} .. against {want[:5]} .."
    # the batch is the loop of single calls
    for qi in sorted({0, case.nq - 1}):
        assert bits32(vb.lookup_top_messages_by_embedding(qs[qi], k, tc.threshold_of(case, qi), handle)) == bits32(got[qi]), (case.name, qi)
    # the host collapse is the native route
    eng.set_option("top_messages", 0)
    try:
        host = vb.lookup_top_messages_by_embeddings(qs, k, thr, handle)
    finally:
        eng.set_option("top_messages", 1)
    assert [bits32(h) for h in host] == [bits32(g) for g in got], case.name


# ---- 2. against the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.B_CASES, ids=[c.name for c in tc.B_CASES])
def test_case_against_the_reference(case):
    vb = index(case.corpus)
    vb.set_row_messages(tc.message_map(case.corpus.rows, case.map))
    qs = tc.corpus_arrays(case.corpus)[2][: case.nq]
    got = vb.lookup_top_messages_by_embeddings(qs, tc.case_k(case), tc.case_thresholds(case), case_handle(vb, case))
    for qi in range(case.nq):
        try:
            tc.judge_b(case, qi, [h.item for h in got[qi]], [h.score for h in got[qi]])
        except AssertionError as e:
            raise AssertionError(f"{case.name} q{qi}: {e}") from e


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------------

def test_ties_order_by_message_ordinal_and_the_refinement_runs_on_the_messages():
    v, q = tc.tie_corpus()
    vb = make_index(v, "float32", np.arange(tc.TIE_ROWS)[::-1].copy())  # row r is message 599 - r: row order is not message order
    eng = vb.engine
    eng.set_option("topk_boundary_keys", tc.TIE_BOUNDARY_KEYS)
    got = vb.lookup_top_messages_by_embedding(q, tc.TIE_K, 0.0)
    rounds = eng.get_option("last_topk_refine")
    assert [h.item for h in got] == list(range(tc.TIE_K))
    assert len({np.float32(h.score).tobytes() for h in got}) == 1
    assert np.float32(got[0].score) == np.float32(vb.fuzzy_lookup_embedding(q, 1, 0.0)[0].score)
    assert rounds >= 1, "600 equal keys cannot fit a boundary list of 64 without a refinement round"
    both = vb.lookup_top_messages_by_embeddings(np.stack([q, -q]), tc.TIE_K, [0.0, 0.0])
    assert [h.item for h in both[0]] == [h.item for h in both[1]] == list(range(tc.TIE_K))


# ---- 4. the device-resident form --------------------------------------------------------------------------------------------------------------

def test_device_form_equals_the_host_query_form():
    import torch

    case = next(c for c in tc.CASES if c.corpus.rows == 4099 and c.corpus.dim == 384)
    probe = tc.Case(case.corpus, "sparse", 9, 300, "per_query", "random10")
    vb = index(probe.corpus)
    rm = tc.message_map(probe.corpus.rows, probe.map)
    vb.set_row_messages(rm)
    qs = tc.corpus_arrays(probe.corpus)[2][: probe.nq]
    thr = np.asarray([_native.f32_threshold(t) for t in tc.case_thresholds(probe)], dtype=np.float32)
    handle = vb.row_mask(tc.case_mask(probe))
    vb.lookup_top_messages_by_embedding(qs[0], 1)  # (the map is on the device)
    eng = vb.engine
    dq = torch.from_numpy(qs).cuda()
    for dev_rows in (None, handle.dev_rows):
        m, s, c = eng.search_top_messages(qs, 300, thr, dev_rows=dev_rows)
        for out in (None, torch.empty((probe.nq, 300), dtype=torch.int64).pin_memory()):
            keys = eng.search_top_messages_device(dq, 300, thr, out_keys=out, dev_rows=dev_rows)
            eng.synchronize()
            m2, s2, c2 = _native.decode_keys(keys.cpu().numpy().view(np.uint64))
            np.testing.assert_array_equal(c2, c)
            for qi in range(probe.nq):
                np.testing.assert_array_equal(m2[qi, : c[qi]], m[qi, : c[qi]])
                np.testing.assert_array_equal(s2[qi, : c[qi]].view(np.uint32), s[qi, : c[qi]].view(np.uint32))
    assert c.max() > 0 and c.min() == 0  # (a threshold above every score is among the nine)
    # n_messages beyond every ordinal in use: the same answer, the extra slots stay empty
    want = eng.search_top_messages(qs, 300, thr)
    rc = eng.lib.tavb_set_row_messages(eng._h, ctypes.c_void_p(eng.row_messages.data_ptr()), len(rm), int(rm.max()) + 1 + 1000)
    assert rc == 0
    try:
        more = eng.search_top_messages(qs, 300, thr)
    finally:
        eng.set_row_messages(rm)
    np.testing.assert_array_equal(want[2], more[2])
    for qi in range(probe.nq):
        np.testing.assert_array_equal(want[0][qi, : want[2][qi]], more[0][qi, : want[2][qi]])
        np.testing.assert_array_equal(want[1][qi, : want[2][qi]].view(np.uint32), more[1][qi, : want[2][qi]].view(np.uint32))


# ---- 5. row edits -----------------------------------------------------------------------------------------------------------------------------

def test_after_row_edits_the_answer_is_a_fresh_index():
    case = tc.Case(tc.CORPORA[6], "chunks3", 3, 25, "zero", "none")
    v, _, qs = tc.corpus_arrays(case.corpus)
    v = np.nan_to_num(v, nan=0.0)
    rm = tc.message_map(case.corpus.rows, case.map)
    vb = make_index(v, case.corpus.dtype, rm)
    before = vb.lookup_top_messages_by_embeddings(qs[:3], 25, 0.0)
    extra = tc.corpus_arrays(tc.CORPORA[9])[0][:40]
    new_msgs = np.arange(40, dtype=np.int64) // 2 + 5000
    at = np.sort(np.random.default_rng(9895).choice(len(v) + 1, size=40))
    assert vb.insert_rows(at, extra, row_messages=new_msgs) == 40
    model_v = np.insert(v, at, extra, axis=0)
    model_rm = np.insert(rm, at, new_msgs)
    fresh = make_index(model_v, case.corpus.dtype, model_rm)
    got = vb.lookup_top_messages_by_embeddings(qs[:3], 25, 0.0)
    assert [bits32(g) for g in got] == [bits32(g) for g in fresh.lookup_top_messages_by_embeddings(qs[:3], 25, 0.0)]
    gone = np.zeros(len(model_v), dtype=bool)
    gone[:: 7] = True
    gone[[h.item * 3 for h in before[0][:5]]] = True  # rows of the best messages among them
    assert vb.remove_rows(gone) == int(gone.sum())
    fresh = make_index(model_v[~gone], case.corpus.dtype, model_rm[~gone])
    got = vb.lookup_top_messages_by_embeddings(qs[:3], 25, [0.0, 0.5, 0.52])
    want = fresh.lookup_top_messages_by_embeddings(qs[:3], 25, [0.0, 0.5, 0.52])
    assert [bits32(g) for g in got] == [bits32(w) for w in want] and len(got[0]) == 25


# ---- 6. errors and fallbacks ------------------------------------------------------------------------------------------------------------------

def test_errors_and_fallbacks():
    case = tc.Case(tc.CORPORA[6], "holes", 2, 10, "zero", "none")
    v, _, qs = tc.corpus_arrays(case.corpus)
    rm = tc.message_map(case.corpus.rows, case.map)
    vb = make_index(v, case.corpus.dtype)
    with pytest.raises(RuntimeError, match="set_row_messages"):
        vb.lookup_top_messages_by_embedding(qs[0], 5)
    eng = vb.engine
    with pytest.raises(_native.TavbError, match="no row -> message map"):
        eng.search_top_messages(qs[:1], 5, 0.0)
    eng.set_row_messages(rm[:-1])
    with pytest.raises(ValueError, match="covers 999 rows, the corpus has 1000"):
        eng.search_top_messages(qs[:1], 5, 0.0)
    eng.set_row_messages(rm)
    for k in (0, _native.MAX_LARGE_K + 1):
        with pytest.raises(ValueError, match="k must be"):
            eng.search_top_messages(qs[:1], k, 0.0)
    assert eng.lib.tavb_search_top_messages_device(eng._h, None, 1, 5, None, None, 0, None) == -1
    vb.set_row_messages(rm)
    # K = 0 (every message) and K beyond 16384 take the host collapse and still answer
    ten = vb.lookup_top_messages_by_embedding(qs[0], 10, 0.0)
    every = vb.lookup_top_messages_by_embedding(qs[0], 0, 0.0)
    beyond = vb.lookup_top_messages_by_embedding(qs[0], _native.MAX_LARGE_K + 1, 0.0)
    n_msgs = len(set(rm[(rm >= 0) & ~np.isnan(v).any(axis=1)].tolist()))
    assert len(every) == len(beyond) == n_msgs and bits32(every) == bits32(beyond) and bits32(every[:10]) == bits32(ten)
    assert bits32(vb.lookup_top_messages_by_embedding(qs[0], n_msgs, 0.0)) == bits32(every)
    # a stale RowMask is refused as elsewhere
    handle = vb.row_mask(np.ones(len(vb), dtype=bool))
    assert len(vb.lookup_top_messages_by_embedding(qs[0], 10, 0.0, handle)) == 10
    vb.remove_rows([3])
    with pytest.raises(ValueError, match="build it again|covers"):
        vb.lookup_top_messages_by_embedding(qs[0], 10, 0.0, handle)


# ---- 7. the lookup this call exists for ---------------------------------------------------------------------------------------------------------

def test_five_messages_where_the_row_lookup_returns_fewer():
    v, q, rm = tc.motive_corpus()
    vb = make_index(v, "float32", rm)
    rows = vb.lookup_messages_by_embedding(q, 5)
    top = vb.lookup_top_messages_by_embedding(q, 5)
    assert len(rows) < 5, "the best 5 chunk rows belong to fewer than 5 messages"
    assert len(top) == 5 and len({h.item for h in top}) == 5
    assert top[0].item == rows[0].item == tc.MOTIVE_NEAR
    assert np.float32(top[0].score).tobytes() == np.float32(rows[0].score).tobytes()
    assert bits32(adapters.lookup_top_messages(vb, q, rm, 5)) == bits32(top)
    assert bits32(adapters.lookup_top_messages(vb, q, rm, 5, scope=[tc.MOTIVE_NEAR, 3])) == bits32([h for h in vb.lookup_top_messages_by_embedding(q, 40) if h.item in (tc.MOTIVE_NEAR, 3)])
