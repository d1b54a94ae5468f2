"""GPU suite: top-k distinct messages on the 32/64-query MFMA tile -- the top-messages form of `skinny_scan_kernel` behind
tavb_search_top_messages_tile / _device, under `VectorBase.lookup_top_messages_by_embedding(s)` with engine option "top_messages_tile".
The table is tests/top_messages_tile_cases.py; tests/test_top_messages_tile_host.py pins it on the CPU.  The route is forced with
option 2 unless a test says otherwise.

  1. every case, per query, against the reference's arithmetic (`top_messages_tile_cases.judge`: scores within SCORE_TOL, order, the
     reference's ordinals up to near-ties decided in float64, the reference's count where no message sits at the threshold);
  2. exact invariants of the tile: an all-ones mask is the unmasked call bit for bit, two identical calls agree, the device form is the
     host form, and where at most 64 rows are allowed the answer is the tile's own lists (the ordinary masked lookup on the 32/64-query
     tile at max_hits = 64) collapsed in numpy, bit for bit;
  3. "masked_route", "last_tier" and "last_skinny_kernel" report what the table expects;
  4. option 0 is today's answer bit for bit; option 1 follows tavb_plan_top_messages_tile;
  5. argument errors, each with its message;
  6. through the class and `adapters.lookup_top_messages`, also after `insert_rows` and `remove_rows`, against a fresh index."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import top_messages_tile_cases as tc
from tests.fakes import NullModel
from tests.synth import make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

pytestmark = pytest.mark.gpu

_state: dict = {}


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def make_index(v, dtype, rm=None, tile=2):
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    if rm is not None:
        vb.set_row_messages(rm)
    if tile is not None:
        vb.engine.set_option("top_messages_tile", tile)
    return vb


def index(corpus: tc.Corpus):
    """One VectorBase per corpus, built once, the tile forced; the case sets its map."""
    if corpus not in _state:
        _state[corpus] = make_index(tc.corpus_arrays(corpus)[0], corpus.dtype)
    return _state[corpus]


def case_handle(vb, case):
    mask = tc.case_mask(case)
    return None if mask is None else vb.row_mask(mask)


def triples(out, nq):
    """(messages, scores, counts) of an Engine call -> per query [(message, score bits)]."""
    m, s, c = out
    return [list(zip(m[q, : c[q]].tolist(), s[q, : c[q]].view(np.uint32).tolist())) for q in range(nq)]


# ---- 1. + 3. every case against the reference, and what the route reports -------------------------------------------------------------

@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_case_against_the_reference(case):
    vb = index(case.corpus)
    vb.set_row_messages(tc.message_map(case.corpus.rows, case.map))
    qs = tc.corpus_arrays(case.corpus)[2][: case.nq]
    handle = case_handle(vb, case)
    eng = vb.engine
    assert eng.get_option("top_messages_tile") == 2
    before = eng.get_option("topk_scores_bytes")
    if case.scores_bytes:
        eng.set_option("topk_scores_bytes", case.scores_bytes)
    eng.set_option("mfma_splits", 0)
    try:
        got = vb.lookup_top_messages_by_embeddings(qs, tc.case_k(case), tc.case_thresholds(case), handle)
        route, tier, kern = eng.get_option("masked_route"), eng.get_option("last_tier"), eng.get_option("last_skinny_kernel")
        again = vb.lookup_top_messages_by_embeddings(qs, tc.case_k(case), tc.case_thresholds(case), handle)
    finally:
        eng.set_option("topk_scores_bytes", before)
    assert len(got) == case.nq
    if case.mask == "empty":
        assert all(g == [] for g in got)
        return
    assert (route, tier, kern) == (10, 5, tc.expected_kernel(case)), case.name
    assert [bits32(g) for g in got] == [bits32(a) for a in again], f"{case.name}: two identical calls differ"
    for qi in range(case.nq):
        try:
            tc.judge(case, qi, [h.item for h in got[qi]], [h.score for h in got[qi]])
        except AssertionError as e:
            raise AssertionError(f"{case.name} q{qi}: {e}") from e


# ---- 2. exact invariants of the tile --------------------------------------------------------------------------------------------------

INVARIANT_CASES = [c for c in tc.CASES if c.mask == "none" and c.thresholds != "above"][:: 3] + [c for c in tc.CASES if c.scores_bytes]


@pytest.mark.parametrize("case", INVARIANT_CASES, ids=[c.name for c in INVARIANT_CASES])
def test_all_ones_mask_and_device_form_equal_the_unmasked_host_call(case):
    import torch

    vb = index(case.corpus)
    vb.set_row_messages(tc.message_map(case.corpus.rows, case.map))
    vb.lookup_top_messages_by_embedding(tc.corpus_arrays(case.corpus)[2][0], 1)  # (the map is on the device)
    qs = tc.corpus_arrays(case.corpus)[2][: case.nq]
    eng, k = vb.engine, tc.case_k(case)
    t = tc.case_thresholds(case)
    thr = np.asarray([_native.f32_threshold(x) for x in (t if isinstance(t, list) else [t] * case.nq)], dtype=np.float32)
    want = triples(eng.search_top_messages_tile(qs, k, thr), case.nq)
    ones = vb.row_mask(np.ones(case.corpus.rows, dtype=bool))
    assert triples(eng.search_top_messages_tile(qs, k, thr, dev_bits=ones.dev_bits, span=ones.span), case.nq) == want
    dq = torch.from_numpy(qs).cuda()
    for out in (None, torch.empty((case.nq, k), dtype=torch.int64).pin_memory()):
        keys = eng.search_top_messages_tile_device(dq, k, thr, out_keys=out)
        eng.synchronize()
        assert triples(_native.decode_keys(keys.cpu().numpy().view(np.uint64)), case.nq) == want
    keys = eng.search_top_messages_tile_device(dq, k, thr, dev_bits=ones.dev_bits, span=ones.span)
    eng.synchronize()
    assert triples(_native.decode_keys(keys.cpu().numpy().view(np.uint64)), case.nq) == want


FEW_ROWS = [(c, nq) for c in tc.CORPORA if c.rows >= 31 for nq in ((5, 33) if c.rows in (31, 257, 4099) else (64,))]


@pytest.mark.parametrize("corpus,nq", FEW_ROWS, ids=[f"{c.name}-q{nq}" for c, nq in FEW_ROWS])
def test_at_most_64_allowed_rows_equal_the_tiles_own_lists_collapsed(corpus, nq):
    """The ordinary masked lookup forced onto the 32/64-query tile at max_hits = 64 returns every allowed passing row with the tile's own
    score; collapsed in numpy that is the top-messages answer, bit for bit -- the same K loop, the same admission test."""
    vb = index(corpus)
    rm = tc.message_map(corpus.rows, "chunks3" if nq != 5 else "holes")
    vb.set_row_messages(rm)
    qs = tc.corpus_arrays(corpus)[2][:nq]
    vb.lookup_top_messages_by_embedding(qs[0], 1)  # (the map is on the device)
    allowed = np.zeros(corpus.rows, dtype=bool)
    pick = np.random.default_rng(corpus.seed + 11).choice(corpus.rows, size=min(corpus.rows, 64), replace=False)
    allowed[pick] = True
    allowed[-1] = allowed[corpus.rows // 3] = True  # the last row (a partial block of the map) and the NaN row among them
    allowed[np.flatnonzero(allowed)[64:]] = False
    handle = vb.row_mask(allowed)
    eng = vb.engine
    thr = np.asarray([(0.0, tc.tenth_threshold(corpus), 0.5)[i % 3] for i in range(nq)], dtype=np.float32)
    rows, scs, cnts = eng.search_masked_batch(qs, handle.dev_bits, 64, thr, span=handle.span)
    assert eng.get_option("masked_route") == 2
    got = triples(eng.search_top_messages_tile(qs, 10, thr, dev_bits=handle.dev_bits, span=handle.span), nq)
    for qi in range(nq):
        m, s = tc.collapse(rows[qi, : cnts[qi]], scs[qi, : cnts[qi]], rm, 10)
        assert got[qi] == list(zip(m.tolist(), s.view(np.uint32).tolist())), f"{corpus.name} q{qi}"


# ---- 3. route reporting ---------------------------------------------------------------------------------------------------------------

def test_the_route_reports_itself():
    corpus = next(c for c in tc.CORPORA if c.rows == 513 and c.dim == 1536)
    vb = index(corpus)
    vb.set_row_messages(tc.message_map(corpus.rows, "chunks3"))
    qs = tc.corpus_arrays(corpus)[2]
    eng = vb.engine
    for nq, kern in ((1, 12832), (32, 12832), (33, 12864), (129, 12832)):  # (129 = 64 + 64 + 1: the last launch is a 32-query tile)
        vb.lookup_top_messages_by_embeddings(qs[:nq], 70, 0.0)
        assert (eng.get_option("masked_route"), eng.get_option("last_tier"), eng.get_option("last_skinny_kernel")) == (10, 5, kern), nq
    eng.set_option("mfma_sched", 9)  # 64-byte K steps on rows of a multiple of 128 bytes
    try:
        vb.lookup_top_messages_by_embeddings(qs[:33], 70, 0.0)
        assert eng.get_option("last_skinny_kernel") == 6464
    finally:
        eng.set_option("mfma_sched", 0)
    handle = vb.row_mask(tc.case_mask(tc.Case(corpus, "chunks3", 2, 10, "zero", "range")))
    vb.lookup_top_messages_by_embeddings(qs[:2], 10, 0.0, handle)
    assert eng.get_option("masked_route") == 10
    vb.fuzzy_lookup_embeddings_masked(qs[:2], handle, 10, 0.0)
    assert eng.get_option("masked_route") != 10


# ---- 4. the option and the plan -------------------------------------------------------------------------------------------------------

def test_option_0_is_todays_answer_and_option_1_follows_the_plan():
    corpus = next(c for c in tc.CORPORA if c.rows == 2049 and c.dtype == "float32")
    v, _, qs = tc.corpus_arrays(corpus)
    rm = tc.message_map(corpus.rows, "holes")
    vb = make_index(v, corpus.dtype, rm, tile=None)  # the option as the engine ships it
    eng = vb.engine
    assert eng.get_option("top_messages_tile") == 0, "the default is 0"
    assert eng.get_option("top_messages_tile_min_batch") == _native.TOP_MESSAGES_TILE_MIN_BATCH
    handle = vb.row_mask(tc.case_mask(tc.Case(corpus, "holes", 2, 10, "zero", "random50")))
    for h in (None, handle):
        got = vb.lookup_top_messages_by_embeddings(qs[:17], 30, 0.0, h)
        assert eng.get_option("masked_route") != 10
        want = triples(eng.search_top_messages(qs[:17], 30, np.zeros(17, np.float32), dev_rows=None if h is None else h.dev_rows), 17)
        assert [bits32(g) for g in got] == want
    eng.set_option("top_messages_tile", 1)
    eng.set_option("mask_tile_min_bytes", 0)
    seen = set()
    for nq in (1, 7, 8, 17, 64):
        for h in (None, handle):
            vb.fuzzy_lookup_embeddings(qs[:2], 5, 0.0)  # (two queries on the streaming scan in between: "last_tier" leaves 5)
            assert eng.get_option("last_tier") != 5
            vb.lookup_top_messages_by_embeddings(qs[:nq], 30, 0.0, h)
            allowed, span = (corpus.rows, corpus.rows) if h is None else (h.count, h.span[1] + 1 - h.span[0] // 256 * 256)
            plan = _native.plan_top_messages_tile(nq, corpus.dim, _native.TAVB_F32, allowed, span, min_bytes=0)
            if h is None:
                assert plan == (nq >= _native.TOP_MESSAGES_TILE_MIN_BATCH == 8)
            took = eng.get_option("last_tier") == 5
            assert took == plan, (nq, h is None)
            seen.add((h is None, plan))
    assert seen == {(True, True), (True, False), (False, True), (False, False)}  # (a 50 % mask under 8 queries: one pass over half the rows against one pass over all of them)
    eng.set_option("top_messages_tile_min_batch", 1)
    vb.lookup_top_messages_by_embeddings(qs[:1], 30, 0.0)
    assert eng.get_option("masked_route") == 10 and eng.get_option("last_tier") == 5


# ---- 5. argument errors ---------------------------------------------------------------------------------------------------------------

def test_argument_errors_carry_their_messages():
    corpus = next(c for c in tc.CORPORA if c.rows == 513 and c.dtype == "float32")
    v, _, qs = tc.corpus_arrays(corpus)
    rm = tc.message_map(corpus.rows, "chunks3")
    vb = make_index(v, corpus.dtype)
    eng = vb.engine
    with pytest.raises(_native.TavbError, match="no row -> message map"):
        eng.search_top_messages_tile(qs[:2], 5, 0.0)
    eng.set_row_messages(rm)
    for k in (0, _native.MAX_LARGE_K + 1):
        with pytest.raises(ValueError, match="k must be"):
            eng.search_top_messages_tile(qs[:2], k, 0.0)
    handle = vb.row_mask(np.ones(corpus.rows, dtype=bool))
    q = np.ascontiguousarray(qs[:2])
    thr = np.zeros(2, np.float32)
    m, s, c = np.zeros((2, 5), np.int64), np.zeros((2, 5), np.float32), np.zeros(2, np.int32)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    args = (ptr(m), ptr(s), ptr(c))
    odd = ctypes.c_void_p(handle.dev_bits.data_ptr() + 2)
    assert eng.lib.tavb_search_top_messages_tile(eng._h, ptr(q), 2, 5, ptr(thr), odd, corpus.rows, 0, corpus.rows - 1, *args) != 0
    assert b"misaligned mask" in eng.lib.tavb_last_error()
    bits = ctypes.c_void_p(handle.dev_bits.data_ptr())
    assert eng.lib.tavb_search_top_messages_tile(eng._h, ptr(q), 2, 5, ptr(thr), bits, corpus.rows + 1, 0, corpus.rows - 1, *args) != 0
    assert b"the mask covers" in eng.lib.tavb_last_error()
    assert eng.lib.tavb_search_top_messages_tile(eng._h, ptr(q), 2, 5, ptr(thr), bits, corpus.rows, 0, corpus.rows, *args) != 0
    assert b"outside the corpus" in eng.lib.tavb_last_error()
    assert eng.lib.tavb_search_top_messages_tile(eng._h, None, 2, 5, ptr(thr), None, 0, 0, 0, *args) != 0
    assert b"null argument" in eng.lib.tavb_last_error()
    # rows of 8 floats are 32 bytes: no K step of the tile
    narrow = make_index(np.ascontiguousarray(v[:, :8]), "float32", rm)
    narrow.engine.set_row_messages(rm)
    with pytest.raises(_native.TavbError, match="multiple of 64 bytes"):
        narrow.engine.search_top_messages_tile(np.ascontiguousarray(qs[:2, :8]), 5, 0.0)
    # ... and the class does not send such a corpus there, whatever the option says
    got = narrow.lookup_top_messages_by_embeddings(np.ascontiguousarray(qs[:2, :8]), 5, 0.0)
    assert narrow.engine.get_option("masked_route") != 10 and len(got[0]) == 5


# ---- 6. through the class and the adapter, and after row edits ------------------------------------------------------------------------

def test_class_adapter_and_row_edits_against_a_fresh_index():
    corpus = next(c for c in tc.CORPORA if c.rows == 513 and c.dtype == "float16")
    v, _, qs = tc.corpus_arrays(corpus)
    v = np.nan_to_num(v, nan=0.0)
    rm = tc.message_map(corpus.rows, "chunks3")
    vb = make_index(v, corpus.dtype, rm)
    eng = vb.engine
    nq, k = 33, 70

    def judge_all(got, model_v, model_rm, mask, thr):
        held = model_v.astype(np.float16).astype(np.float32)
        for qi in range(len(got)):
            b32, b64 = tc.best_of_arrays(held, qs[qi], model_rm, mask)
            tc.judge_lists(b32, b64, corpus.dim, k, thr, [h.item for h in got[qi]], [h.score for h in got[qi]], f"q{qi}")

    got = vb.lookup_top_messages_by_embeddings(qs[:nq], k, 0.0)
    assert eng.get_option("masked_route") == 10
    judge_all(got, v, rm, None, 0.0)
    one = adapters.lookup_top_messages(vb, qs[0], rm, k)
    assert bits32(one) == bits32(vb.lookup_top_messages_by_embedding(qs[0], k)) and eng.get_option("masked_route") == 10
    scope = list(range(0, 100, 3))
    scoped = adapters.lookup_top_messages(vb, qs[:nq], rm, k, 0.0, scope=scope)
    assert eng.get_option("masked_route") == 10
    judge_all(scoped, v, rm, np.isin(rm, scope), 0.0)
    extra = make_queries(40, corpus.dim, 9994)  # 40 more unit rows
    new_msgs = np.arange(40, dtype=np.int64) // 2 + 500
    at = np.sort(np.random.default_rng(9995).choice(len(v) + 1, size=40))
    assert vb.insert_rows(at, extra, row_messages=new_msgs) == 40
    model_v, model_rm = np.insert(v, at, extra, axis=0), np.insert(rm, at, new_msgs)
    got = vb.lookup_top_messages_by_embeddings(qs[:nq], k, 0.0)
    assert eng.get_option("masked_route") == 10
    judge_all(got, model_v, model_rm, None, 0.0)
    fresh = make_index(model_v, corpus.dtype, model_rm)
    assert [bits32(g) for g in got] == [bits32(f) for f in fresh.lookup_top_messages_by_embeddings(qs[:nq], k, 0.0)]
    gone = np.zeros(len(model_v), dtype=bool)
    gone[:: 7] = True
    assert vb.remove_rows(gone) == int(gone.sum())
    model_v, model_rm = model_v[~gone], model_rm[~gone]
    got = vb.lookup_top_messages_by_embeddings(qs[:nq], k, 0.5)
    assert eng.get_option("masked_route") == 10
    judge_all(got, model_v, model_rm, None, 0.5)
    fresh = make_index(model_v, corpus.dtype, model_rm)
    assert [bits32(g) for g in got] == [bits32(f) for f in fresh.lookup_top_messages_by_embeddings(qs[:nq], k, 0.5)]
