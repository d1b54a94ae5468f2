"""GPU suite: top-k distinct messages under one scope per query in one submission -- `ScopedMessageMaxSink` behind
tavb_search_top_messages_scoped / _device, under `VectorBase.lookup_top_messages_by_embeddings_scoped` and
`adapters.lookup_top_messages_in_scopes`.  The table is tests/top_messages_scoped_cases.py; tests/test_top_messages_scoped_host.py pins
it on the CPU.  Answers are compared bit for bit: message ordinals, float32 score bits, counts.

  1. every case equals the loop of `lookup_top_messages_by_embedding(e_i, K, t_i, scope_i)`;
  2. every case equals expected answer A per query: the library's own row scores, `fuzzy_lookup_embedding_masked(e_i, scope_i, len(vb),
     t_i)`, collapsed by `top_messages_cases.collapse`;
  3. "masked_route" reads 9 exactly where the table's `expect_native` says so;
  4. "top_messages_scoped" = 0 gives the same lists;
  5. the device form equals the host form;
  6. nine queries under "topk_scores_bytes" at its floor (sub-groups with bit0 > 0) equal the answer at the default, and
     "last_topk_refine" is readable afterwards;
  7. one case per corpus against the reference's arithmetic (`judge_b` per query over that query's own scope);
  8. after `remove_rows(..., carry=handles)` and `insert_rows(..., row_messages=..., carry=handles)` the scoped answer is a fresh index's
     over numpy's result;
  9. errors: no map, a map that does not cover the corpus, a stale handle, K = 0 and K = 16385 (the loop's lists)."""

from __future__ import annotations

import numpy as np
import pytest

from tests import top_messages_scoped_cases as ts
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native, adapters

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


def index(corpus: ts.Corpus):
    """One VectorBase per corpus, built once; the case sets its map."""
    if corpus not in _state:
        _state[corpus] = make_index(ts.corpus_arrays(corpus)[0], corpus.dtype)
    return _state[corpus]


def case_scope_objects(vb, case):
    """(the scopes as the case hands them to the class, one `RowMask` per query for the per-query calls): an object that appears several
    times in the case's scopes appears as often in both."""
    bools = ts.case_scopes(case)
    specs = ts.scope_specs(case) if case.form == "message_handles" else bools
    made: dict[int, RowMask] = {}
    for spec, b in zip(specs, bools):
        if id(spec) in made:
            continue
        if case.form != "message_handles":
            made[id(spec)] = vb.row_mask(b)
        elif spec[0] == "messages":
            made[id(spec)] = vb.message_mask(spec[1])
        else:
            made[id(spec)] = vb.range_mask(spec[1], of="messages")
        assert made[id(spec)].count == int(b.sum()), case.name
    handles = [made[id(spec)] for spec in specs]
    if case.form == "raw":
        return bools, handles
    if case.form == "host_only":  # one handle with the row list but without the packed mask, as a library before the scoped routes hands out
        h = handles[1]
        lame = RowMask(vb, h.rows, h.count, dev_rows=h.dev_rows)
        handles = [lame if x is h else x for x in handles]
        assert lame.dev_bits is None
    return handles, handles


def reset_route(vb, q):
    """A masked lookup on the row list: "masked_route" reads 1 afterwards."""
    vb.fuzzy_lookup_embedding_masked(q, vb.row_mask(np.ones(len(vb), dtype=bool)), 1, 0.0)
    assert vb.engine.get_option("masked_route") == 1


def answer_a(vb, case, q, qi, handle):
    """Expected answer A: the library's own exact scores of every passing row of the query's own scope, collapsed in numpy."""
    hits = vb.fuzzy_lookup_embedding_masked(q, handle, len(vb), ts.threshold_of(case, qi))
    m, s = ts.collapse([h.item for h in hits], [h.score for h in hits], ts.message_map(case.corpus.rows, case.map), ts.case_k(case))
    return list(zip(m.tolist(), s.view(np.uint32).tolist()))


def check_case(vb, case):
    """Checks 1 - 4 on an index that holds the case's corpus and map; returns the scoped answer."""
    qs = ts.case_queries(case)
    scopes, handles = case_scope_objects(vb, case)
    k, thr = ts.case_k(case), ts.case_thresholds(case)
    eng = vb.engine
    assert eng.get_option("top_messages") == 1 and eng.get_option("top_messages_scoped") == 1
    reset_route(vb, qs[0])
    got = vb.lookup_top_messages_by_embeddings_scoped(qs, scopes, k, thr)
    route = eng.get_option("masked_route")
    assert len(got) == case.nq
    assert route == (9 if ts.expect_native(case) else 1), f"{case.name}: masked_route {route}, expect_native {ts.expect_native(case)}"
    for qi in range(case.nq):
        loop = bits32(vb.lookup_top_messages_by_embedding(qs[qi], k, ts.threshold_of(case, qi), handles[qi]))
        assert bits32(got[qi]) == loop, f"{case.name} q{qi}: {bits32(got[qi])[:4]} .. against the loop's {loop[:4]} .."
        want = answer_a(vb, case, qs[qi], qi, handles[qi])
        assert bits32(got[qi]) == want, f"{case.name} q{qi}: {bits32(got[qi])[:4]} .. against A's {want[:4]} .."
    reset_route(vb, qs[0])
    eng.set_option("top_messages_scoped", 0)
    try:
        looped = vb.lookup_top_messages_by_embeddings_scoped(qs, scopes, k, thr)
        assert eng.get_option("masked_route") == 1
    finally:
        eng.set_option("top_messages_scoped", 1)
    assert [bits32(x) for x in looped] == [bits32(x) for x in got], case.name
    return got


# ---- 1 - 4. every case ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ts.TABLE_CASES, ids=[c.name for c in ts.TABLE_CASES])
def test_case_against_the_loop_and_the_librarys_own_scores(case):
    vb = index(case.corpus)
    vb.set_row_messages(ts.message_map(case.corpus.rows, case.map))
    got = check_case(vb, case)
    if case.note == "hand2":  # one message, disjoint scopes: each query's single score is its own scope's best row
        assert all(len(g) == 1 and g[0].item == 0 for g in got) and len({bits32(g)[0][1] for g in got}) > 1


def test_adopted_corpus_message_ordinals_do_not_carry_the_ordinal_base():
    import torch

    case = ts.HAND["5"]
    _, held, _ = ts.corpus_arrays(case.corpus)
    held = np.nan_to_num(held, nan=0.0)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    vb.adopt_device_corpus(torch.from_numpy(held.astype(np.float16)).cuda(), ordinal_base=ts.ORDINAL_BASE)
    vb.set_row_messages(ts.message_map(case.corpus.rows, case.map))
    eng = vb.engine
    assert eng.ordinal_base == ts.ORDINAL_BASE
    got = check_case(vb, case)
    n = ts.n_messages(case)
    assert any(got) and all(0 <= h.item < n for g in got for h in g)
    handles = [vb.row_mask(s) for s in ts.case_scopes(case)]
    t = np.asarray([_native.f32_threshold(x) for x in ts.case_thresholds(case)], dtype=np.float32)
    m, s, c = eng.search_top_messages_scoped(ts.case_queries(case), [h.dev_bits for h in handles], ts.case_k(case), t)
    for qi in range(case.nq):
        assert m[qi, : c[qi]].tolist() == [h.item for h in got[qi]]


# ---- 5. the device form -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["1b", "2", "4", "6c"])
def test_device_form_equals_the_host_form(key):
    import torch

    case = ts.HAND[key]
    vb = index(case.corpus)
    vb.set_row_messages(ts.message_map(case.corpus.rows, case.map))
    qs, k = ts.case_queries(case), ts.case_k(case)
    _, handles = case_scope_objects(vb, case)
    vb.lookup_top_messages_by_embedding(qs[0], 1)  # (the map is on the device)
    eng = vb.engine
    t = np.broadcast_to(np.asarray(ts.case_thresholds(case), dtype=np.float64), (case.nq,))
    t = np.asarray([_native.f32_threshold(x) for x in t], dtype=np.float32)
    masks = [h.dev_bits for h in handles]
    m, s, c = eng.search_top_messages_scoped(qs, masks, k, t)
    assert eng.get_option("masked_route") == 9 and c.max() > 0
    dq = torch.from_numpy(qs).cuda()
    for out in (None, torch.empty((case.nq, k), dtype=torch.int64).pin_memory()):
        keys = eng.search_top_messages_scoped_device(dq, masks, k, t, out_keys=out)
        eng.synchronize()
        m2, s2, c2 = _native.decode_keys(keys.cpu().numpy().view(np.uint64))
        np.testing.assert_array_equal(c2, c)
        for qi in range(case.nq):
            np.testing.assert_array_equal(m2[qi, : c[qi]], m[qi, : c[qi]])
            np.testing.assert_array_equal(s2[qi, : c[qi]].view(np.uint32), s[qi, : c[qi]].view(np.uint32))
    assert eng.get_option("last_topk_refine") >= 0


# ---- 6. sub-groups of a pass ----------------------------------------------------------------------------------------------------------------------

def test_subgroups_under_the_floor_of_topk_scores_bytes_equal_the_default():
    case = ts.HAND["3"]
    vb = index(case.corpus)
    vb.set_row_messages(ts.message_map(case.corpus.rows, case.map))
    qs, k, thr = ts.case_queries(case), ts.case_k(case), ts.case_thresholds(case)
    handles = [vb.row_mask(s) for s in ts.case_scopes(case)]
    eng = vb.engine
    default = eng.get_option("topk_scores_bytes")
    assert default > ts.FLOOR_BYTES
    want = vb.lookup_top_messages_by_embeddings_scoped(qs, handles, k, thr)
    eng.set_option("topk_scores_bytes", ts.FLOOR_BYTES)
    try:
        got = vb.lookup_top_messages_by_embeddings_scoped(qs, handles, k, thr)
        assert eng.get_option("masked_route") == 9
        rounds = eng.get_option("last_topk_refine")
    finally:
        eng.set_option("topk_scores_bytes", default)
    assert [bits32(g) for g in got] == [bits32(w) for w in want] and any(got)
    assert isinstance(rounds, int) and rounds >= 0


# ---- 7. against the reference ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ts.B_CASES, ids=[c.name for c in ts.B_CASES])
def test_case_against_the_reference(case):
    vb = index(case.corpus)
    vb.set_row_messages(ts.message_map(case.corpus.rows, case.map))
    scopes, _ = case_scope_objects(vb, case)
    got = vb.lookup_top_messages_by_embeddings_scoped(ts.case_queries(case), scopes, ts.case_k(case), ts.case_thresholds(case))
    assert vb.engine.get_option("masked_route") == 9
    for qi in range(case.nq):
        try:
            ts.judge_b(case, qi, [h.item for h in got[qi]], [h.score for h in got[qi]])
        except AssertionError as e:
            raise AssertionError(f"{case.name} q{qi}: {e}") from e


# ---- 8. row edits ---------------------------------------------------------------------------------------------------------------------------------

def test_after_row_edits_with_carried_handles_the_answer_is_a_fresh_index():
    corpus = ts.CORPORA[8]  # 1000 x 8 fp32
    v, _, qs = ts.corpus_arrays(corpus)
    v = np.nan_to_num(v, nan=0.0)
    rm = ts.message_map(corpus.rows, "interleaved")
    vb = make_index(v, corpus.dtype, rm)
    rng = np.random.default_rng(9795)
    bools = [rng.random(len(v)) < p for p in (0.5, 0.1, 0.5)] + [np.zeros(len(v), dtype=bool)]
    handles = [vb.row_mask(b) for b in bools]
    thr = [0.0, 0.5, 0.52, 0.0]

    def fresh_answer(model_v, model_rm):
        fresh = make_index(model_v, corpus.dtype, model_rm)
        return [bits32(fresh.lookup_top_messages_by_embedding(qs[i], 25, thr[i], bools[i])) for i in range(4)]

    gone = np.zeros(len(v), dtype=bool)
    gone[::7] = True
    assert vb.remove_rows(gone, carry=handles) == int(gone.sum())
    v, rm, bools = v[~gone], rm[~gone], [b[~gone] for b in bools]
    got = vb.lookup_top_messages_by_embeddings_scoped(qs[:4], handles, 25, thr)
    assert vb.engine.get_option("masked_route") == 9
    assert [bits32(g) for g in got] == fresh_answer(v, rm) and len(got[0]) == 25 and got[3] == []
    extra = ts.corpus_arrays(ts.CORPORA[10])[0][:40]
    new_msgs = np.arange(40, dtype=np.int64) // 2 + 5000
    at = np.sort(rng.choice(len(v) + 1, size=40))
    assert vb.insert_rows(at, extra, row_messages=new_msgs, carry=handles) == 40
    v, rm, bools = np.insert(v, at, extra, axis=0), np.insert(rm, at, new_msgs), [np.insert(b, at, False) for b in bools]
    got = vb.lookup_top_messages_by_embeddings_scoped(qs[:4], handles, 25, thr)
    assert vb.engine.get_option("masked_route") == 9
    assert [bits32(g) for g in got] == fresh_answer(v, rm) and all(h.item < 5000 for g in got for h in g)


# ---- 9. errors and fallbacks ------------------------------------------------------------------------------------------------------------------------

def test_errors_and_fallbacks():
    corpus = ts.CORPORA[8]
    v, _, qs = ts.corpus_arrays(corpus)
    rm = ts.message_map(corpus.rows, "holes")
    vb = make_index(v, corpus.dtype)
    rng = np.random.default_rng(9796)
    a, b = vb.row_mask(rng.random(len(v)) < 0.5), vb.row_mask(rng.random(len(v)) < 0.3)
    with pytest.raises(RuntimeError, match="set_row_messages"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], 5)
    eng = vb.engine
    masks = [a.dev_bits, b.dev_bits]
    with pytest.raises(_native.TavbError, match="no row -> message map"):
        eng.search_top_messages_scoped(qs[:2], masks, 5, 0.0)
    eng.set_row_messages(rm[:-1])
    with pytest.raises(ValueError, match="covers 999 rows, the corpus has 1000"):
        eng.search_top_messages_scoped(qs[:2], masks, 5, 0.0)
    eng.set_row_messages(rm)
    for k in (0, _native.MAX_LARGE_K + 1):
        with pytest.raises(ValueError, match="k must be|serves 1 <= k"):
            eng.search_top_messages_scoped(qs[:2], masks, k, 0.0)
    assert eng.lib.tavb_search_top_messages_scoped_device(eng._h, None, 2, None, len(v), 5, None, None) == -1
    assert eng.lib.tavb_search_top_messages_scoped(eng._h, None, 2, None, len(v) + 1, 5, None, None, None, None) == -1
    assert b"the mask covers" in eng.lib.tavb_last_error()
    vb.set_row_messages(rm)
    # K = 0 (every message) and K beyond 16384 loop into the host collapse and still answer: the loop's lists
    for k in (0, _native.MAX_LARGE_K + 1):
        reset_route(vb, qs[0])
        got = vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], k, [0.0, 0.5])
        assert eng.get_option("masked_route") != 9
        assert [bits32(g) for g in got] == [bits32(vb.lookup_top_messages_by_embedding(qs[i], k, t, h)) for i, (t, h) in enumerate(((0.0, a), (0.5, b)))]
        assert len(got[0]) > 25 and bits32(got[0][:25]) == bits32(vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], 25, [0.0, 0.5])[0])
    # the adapter is the class call
    msgs = [1, 2, 3, 50]
    got = adapters.lookup_top_messages_in_scopes(vb, qs[:3], rm, [msgs, a, msgs], 10, 0.0)
    assert eng.get_option("masked_route") == 9
    assert bits32(got[1]) == bits32(vb.lookup_top_messages_by_embedding(qs[1], 10, 0.0, a)) and {h.item for h in got[0]} <= {1, 2, 3, 50}
    # a stale RowMask is refused as elsewhere
    vb.remove_rows([3])
    with pytest.raises(ValueError, match="build it again|covers"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], 5)
