"""GPU suite: scoped message lookups -- `mask_from_messages_kernel` behind tavb_mask_from_messages, and the batched message lookups
tavb_search_messages_masked / tavb_search_messages_batch under `VectorBase.message_mask`, `lookup_messages_by_embedding(s)_masked`,
`lookup_messages_by_embeddings` and `adapters.lookup_messages_in_scope`.  The table is tests/message_scope_cases.py;
tests/test_message_scope_host.py pins it on the CPU.

  1. every mask case: the device words equal the numpy twin of the kernel, whole words (the library is handed words of all ones: the bits
     at or beyond the corpus must come back zero, the word behind the mask untouched); the expansion's rows, count and span match;
  2. `message_mask` + `fuzzy_lookup_embeddings_masked` == the same lookup with the host-built bool mask, bit for bit, on every route;
  3. every lookup case: on the row list (route 1) and the wide filter tile (route 3) the batch equals the per-query
     `lookup_messages_in_subset_by_embedding` over np.flatnonzero(mask) in messages, float32 scores and counts, bit for bit; on the
     32/64-query tile (route 2) the comparison of tests/test_gpu_masked_tile.py, one level up: messages identical except among float32
     near-ties, which a float64 referee decides (`oracle.vectorbase_oracle.check_topk_parity` over the best score per message), scores
     within 1e-5, and the number of messages what the best `max_matches` allowed rows hold, up to rows in a near tie with the last of
     them.  A shape the forced route does not serve (width 72 or max_matches 65 on the tile, fp32 on the wide tile) runs on the row list
     with the same answers.  `masked_route` is asserted in every case;
  4. `lookup_messages_by_embeddings` == the single calls bit for bit where the batch route is bit-exact: 8 queries on the grouped
     streaming scan, 65 on the wide tile of an fp16 corpus; with and without `accept_ordinals`;
  5. an adopted corpus with ordinal_base != 0.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import message_scope_cases as sc
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native, adapters

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


# ---- 1. the mask kernel ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mask_engine():
    eng = _native.Engine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("case", sc.MASK_CASES, ids=[c.name for c in sc.MASK_CASES])
def test_mask_case(mask_engine, case):
    torch = _torch()
    eng = mask_engine
    m = sc.mask_case_map(case)
    eng.set_corpus_tensor(torch.zeros((case.rows, 8), dtype=torch.float32, device="cuda"))
    eng.set_row_messages(m)
    n_bits = int(m.max()) + 1 if (m >= 0).any() else 0
    n_words = (case.rows + 31) // 32
    for name, accept in sc.accept_sets(case.n_messages, case.seed).items():
        want = sc.twin_mask_words(m, case.rows, accept, n_bits)
        flat = np.flatnonzero(sc.isin_mask(m, case.rows, accept))
        # the library itself, over words of all ones with one more behind them
        acc = np.ascontiguousarray(accept, dtype=np.int32)
        raw = torch.full((n_words + 1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc = eng.lib.tavb_mask_from_messages(eng._h, _native._addr(acc) if acc.size else None, acc.size, case.rows, ctypes.c_void_p(raw.data_ptr()))
        assert rc == 0, eng.lib.tavb_last_error()
        eng.synchronize()
        got = raw.cpu().numpy().view(np.uint32)
        assert got[n_words] == 0xFFFFFFFF, f"{case.name} {name}: the word behind the mask was written"
        np.testing.assert_array_equal(got[:n_words], want, err_msg=f"{case.name} {name}")
        # the binding: mask, expansion, count
        dev_rows, count, dev_bits = eng.mask_from_messages(accept)
        np.testing.assert_array_equal(dev_bits.cpu().numpy().view(np.uint32), want, err_msg=f"{case.name} {name}")
        assert count == len(flat) == int(dev_rows.numel()), (case.name, name)
        np.testing.assert_array_equal(dev_rows.cpu().numpy(), flat.astype(np.int32))
        handle = RowMask(object.__new__(VectorBase), case.rows, count, dev_rows=dev_rows, dev_bits=dev_bits)
        assert handle.span == ((int(flat[0]), int(flat[-1])) if len(flat) else None), (case.name, name)


def test_mask_argument_errors():
    torch = _torch()
    eng = _native.Engine(0)
    eng.set_corpus_tensor(torch.zeros((100, 8), dtype=torch.float32, device="cuda"))
    with pytest.raises(_native.TavbError, match="no row -> message map"):
        eng.mask_from_messages([1])
    eng.set_row_messages(np.zeros(99, dtype=np.int64))
    with pytest.raises(ValueError, match="covers 99 rows, the corpus has 100"):
        eng.mask_from_messages([1])
    eng.set_row_messages(np.zeros(100, dtype=np.int64))
    bits = torch.zeros(4, dtype=torch.int32, device="cuda")
    assert eng.lib.tavb_mask_from_messages(eng._h, None, 0, 99, ctypes.c_void_p(bits.data_ptr())) == -1  # not the corpus' rows
    assert eng.lib.tavb_mask_from_messages(eng._h, None, 3, 100, ctypes.c_void_p(bits.data_ptr())) == -1  # a list without an address
    eng.close()


# ---- the lookup corpora ------------------------------------------------------------------------------------------------------------------

_state: dict = {}


def index(corpus: sc.Corpus):
    """(VectorBase with the map set, the rows as the device holds them, 130 queries) per corpus, built once."""
    if corpus.name not in _state:
        v, _ = make_corpus(sc.ROWS, corpus.dim, corpus.seed)
        qs = make_queries(sc.MAX_QUERIES, corpus.dim, corpus.seed + 1)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=corpus.dtype)
        vb.add_embeddings(None, v)
        vb.set_row_messages(sc.lookup_map())
        held = v.astype(np.float16).astype(np.float32) if corpus.dtype == "float16" else v
        _state[corpus.name] = (vb, held, qs)
    return _state[corpus.name]


def force(eng, route: str) -> None:
    tile, wide = sc.ROUTES[route]
    eng.set_option("mask_tile", tile)
    eng.set_option("mask_wide", wide)


def reference(corpus: sc.Corpus, scope: str, max_matches, thresholds: str):
    """The per-query `lookup_messages_in_subset_by_embedding` over np.flatnonzero(mask) for all 130 queries, once per (corpus, scope,
    max_matches, thresholds); thresholds per query repeat with the query's index, so a shorter batch is a prefix."""
    key = (corpus.name, scope, max_matches, thresholds)
    if key not in _state:
        vb, _, qs = index(corpus)
        probe = sc.LookupCase(corpus, "list", sc.MAX_QUERIES, max_matches, scope, thresholds)
        flat = np.flatnonzero(sc.case_mask(probe)).tolist()
        thr = sc.case_thresholds(probe)
        _state[key] = [vb.lookup_messages_in_subset_by_embedding(q, flat, max_matches, thr[i] if isinstance(thr, list) else thr) for i, q in enumerate(qs)]
    return _state[key]


def check_near_ties(name, held, rm, mask, q, k, thr, got):
    """Route 2.  `got`: the messages of one query.  Best score per message over its allowed rows (float32 reference, float64 referee):
    `check_topk_parity` accepts the list when it is the best len(got) messages in order, a different message at a rank only within the
    measured near-tie width, scores within 1e-5.  Then the count: the distinct messages among the allowed rows that are surely among the
    best k (above the k-th by more than that width) <= len(got) <= those among the rows that may be."""
    flat = np.flatnonzero(mask)
    msgs = rm[flat]
    ref32 = vo.cosine_to_score(np.dot(held[flat], q)).astype(np.float32)
    ref64 = vo.scores_f64(held[flat], q)
    n_msg = int(rm.max()) + 1
    best32 = np.full(n_msg, np.nan, dtype=np.float32)
    best64 = np.full(n_msg, -1.0)
    live = msgs >= 0
    for score, table in ((ref32, best32), (ref64, best64)):
        order = np.argsort(score[live], kind="stable")  # ascending: the best row of a message is written last
        table[msgs[live][order]] = score[live][order]

    def referee(positions):
        return best64[np.asarray(positions, dtype=np.int64)]

    referee.dim = held.shape[1]
    items, scores = [h.item for h in got], [h.score for h in got]
    width = vo.TIE_EPS
    if got:  # (no message at all: only the count below says whether that is right)
        try:
            rep = vo.check_topk_parity(best32, items, scores, len(got), float(thr), referee=referee)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e
        width = max(rep.tie_width, vo.TIE_EPS)
    passing = ref32 >= np.float32(thr)
    ranked = np.sort(ref64[passing])[::-1]
    kth = ranked[k - 1] if len(ranked) >= k else -np.inf
    edge = max(kth, float(np.float32(thr)))
    sure = live & (ref64 > edge + width)
    maybe = live & (ref64 >= edge - width)
    lo, hi = len(set(msgs[sure].tolist())), len(set(msgs[maybe].tolist()))
    assert lo <= len(got) <= hi, f"{name}: {len(got)} messages, the best {k} allowed rows hold {lo} .. {hi}"


@pytest.mark.parametrize("case", sc.LOOKUP_CASES, ids=[c.name for c in sc.LOOKUP_CASES])
def test_lookup_case(case):
    vb, held, qs = index(case.corpus)
    eng = vb.engine
    rm = sc.lookup_map()
    mask = sc.case_mask(case)
    thr = sc.case_thresholds(case)
    want = reference(case.corpus, case.scope, case.max_matches, case.thresholds)[: case.nq]
    handle = vb.row_mask(mask) if case.scope == "rows" else vb.message_mask(sc.scope_messages(case.scope))
    assert isinstance(handle, RowMask) and handle.count == int(mask.sum())
    if handle.count:
        assert handle.dev_rows is not None and handle.dev_bits is not None
        np.testing.assert_array_equal(handle.dev_rows.cpu().numpy(), np.flatnonzero(mask).astype(np.int32))
    force(eng, case.route)
    try:
        got = vb.lookup_messages_by_embeddings_masked(qs[: case.nq], handle, case.max_matches, thr)
        route = eng.get_option("masked_route")
    finally:
        eng.set_option("mask_tile", 1)
        eng.set_option("mask_wide", 1)
    assert len(got) == case.nq
    if handle.count == 0:
        assert got == [[] for _ in range(case.nq)] == want
        return
    expected = sc.expected_route(case)
    assert route == expected, f"{case.name}: masked_route {route}, expected {expected}"
    k = 10 if case.max_matches is None else case.max_matches
    in_scope = set(rm[mask & (rm >= 0)].tolist())
    for i in range(case.nq):
        t = thr[i] if isinstance(thr, list) else thr
        assert all(h.item in in_scope for h in got[i]), f"{case.name}: query {i} returned a message without an allowed row"
        if expected != 2:
            assert bits32(got[i]) == bits32(want[i]), f"{case.name}: query {i} differs from the sequential lookup"
            continue
        if t > 1:
            assert got[i] == []
            continue
        check_near_ties(f"{case.name} query {i}", held, rm, mask, qs[i], k, t, got[i])
    if case.nq == 1:
        one = vb.lookup_messages_by_embedding_masked(qs[0], handle, case.max_matches, thr if not isinstance(thr, list) else thr[0])
        assert bits32(one) == bits32(want[0])  # (a single query is below every tile's batch: the row list)


# ---- 2. message_mask feeds the chunk-level masked lookups ---------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus", sc.CORPORA, ids=[c.name for c in sc.CORPORA])
@pytest.mark.parametrize("route", list(sc.ROUTES))
def test_message_mask_equals_the_host_built_mask(corpus, route):
    vb, held, qs = index(corpus)
    eng = vb.engine
    rm = sc.lookup_map()
    for scope in ("1%", "50%", "100%"):
        messages = sc.scope_messages(scope)
        mask = sc.isin_mask(rm, sc.ROWS, messages)
        force(eng, route)
        try:
            for nq, k in ((9, 10), (65, 64)):
                a = vb.fuzzy_lookup_embeddings_masked(qs[:nq], vb.message_mask(messages), k, 0.5, as_arrays=True)
                ra = eng.get_option("masked_route")
                b = vb.fuzzy_lookup_embeddings_masked(qs[:nq], mask, k, 0.5, as_arrays=True)
                assert ra == eng.get_option("masked_route")
                assert np.array_equal(a[2], b[2])
                for q in range(nq):
                    m = int(a[2][q])
                    assert np.array_equal(a[0][q, :m], b[0][q, :m]) and np.array_equal(a[1][q, :m].view(np.uint32), b[1][q, :m].view(np.uint32)), (scope, nq, k, q)
        finally:
            eng.set_option("mask_tile", 1)
            eng.set_option("mask_wide", 1)


def test_lookup_messages_in_scope_on_the_device():
    corpus = sc.CORPORA[0]
    vb, held, qs = index(corpus)
    rm = sc.lookup_map()
    scope = sc.scope_messages("50%")
    flat = np.flatnonzero(sc.isin_mask(rm, sc.ROWS, scope)).tolist()
    for max_matches in (None, 5, 40):
        want = [adapters.lookup_messages_in_subset(vb, q, flat, rm, max_matches, 0.5) for q in qs[:9]]
        got = adapters.lookup_messages_in_scope(vb, qs[:9], rm, scope.tolist(), max_matches, 0.5)
        assert [bits32(x) for x in got] == [bits32(x) for x in want]
        assert bits32(adapters.lookup_messages_in_scope(vb, qs[3], rm, vb.message_mask(scope), max_matches, 0.5)) == bits32(want[3])
    assert vb.engine.get_option("masked_route") == 1


# ---- 4. the unscoped batch ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("corpus", sc.CORPORA[:2], ids=[c.name for c in sc.CORPORA[:2]])
def test_batched_message_lookup_on_the_grouped_scan(corpus):
    vb, held, qs = index(corpus)
    eng = vb.engine
    accept = sc.scope_messages("50%").tolist() + [-4, sc.N_MESSAGES + 3]
    eng.set_option("direct_group", 8)
    try:
        for max_matches in (None, 1, 64):
            for acc in (None, accept, []):
                for thr in (0.0, [sc.PER_QUERY_THRESHOLDS[i % 4] for i in range(8)]):
                    got = vb.lookup_messages_by_embeddings(qs[:8], max_matches, thr, accept_ordinals=acc)
                    assert eng.get_option("last_direct") == 4  # the grouped streaming scan + one merge
                    for i in range(8):
                        t = thr[i] if isinstance(thr, list) else thr
                        assert bits32(got[i]) == bits32(vb.lookup_messages_by_embedding(qs[i], max_matches, t, accept_ordinals=acc)), (max_matches, acc is None, i)
    finally:
        eng.set_option("direct_group", 0)


def test_batched_message_lookup_on_the_wide_tile():
    corpus = sc.CORPORA[0]  # fp16
    vb, held, qs = index(corpus)
    eng = vb.engine
    accept = sc.scope_messages("50%").tolist()
    eng.set_option("direct_group_max_nq", 0)  # (on a corpus this small the grouped streaming scan would take 65 queries up to max_matches 64)
    try:
        for max_matches in (10, 65, 256):
            for acc in (None, accept):
                got = vb.lookup_messages_by_embeddings(qs[:65], max_matches, 0.5, accept_ordinals=acc)
                assert eng.get_option("last_tier") == 4 and eng.get_option("last_direct") == 0  # the 128/256-query filter tile + rescoring
                for i in range(65):
                    assert bits32(got[i]) == bits32(vb.lookup_messages_by_embedding(qs[i], max_matches, 0.5, accept_ordinals=acc)), (max_matches, acc is None, i)
    finally:
        eng.set_option("direct_group_max_nq", 128)
    # a narrow scope as a post-filter finds less than the scoped search (the reason the masked form exists)
    narrow = sc.scope_messages("1%")
    post = vb.lookup_messages_by_embeddings(qs[:8], 10, 0.0, accept_ordinals=narrow.tolist())
    scoped = vb.lookup_messages_by_embeddings_masked(qs[:8], vb.message_mask(narrow), 10, 0.0)
    assert all(len(s) >= len(p) for s, p in zip(scoped, post)) and sum(map(len, scoped)) > sum(map(len, post))


# ---- 5. an adopted corpus with an ordinal base ---------------------------------------------------------------------------------------------

def test_adopted_corpus_with_an_ordinal_base():
    torch = _torch()
    corpus = sc.CORPORA[0]
    _, held, qs = index(corpus)
    rm = sc.lookup_map()
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    vb.adopt_device_corpus(torch.from_numpy(held.astype(np.float16)).cuda(), ordinal_base=70_000)
    vb.set_row_messages(rm)
    eng = vb.engine
    assert eng.ordinal_base == 70_000
    messages = sc.scope_messages("50%")
    mask = sc.isin_mask(rm, sc.ROWS, messages)
    flat = np.flatnonzero(mask).tolist()
    handle = vb.message_mask(messages)
    np.testing.assert_array_equal(handle.flat(), np.flatnonzero(mask))
    want = [vb.lookup_messages_in_subset_by_embedding(q, flat, 20, 0.5) for q in qs[:65]]
    for route in sc.ROUTES:
        force(eng, route)
        got = vb.lookup_messages_by_embeddings_masked(qs[:65], handle, 20, 0.5)
        assert eng.get_option("masked_route") == {"list": 1, "tile": 2, "wide": 3}[route]
        for i in range(65):
            if route == "tile":
                check_near_ties(f"base-{route} query {i}", held, rm, mask, qs[i], 20, 0.5, got[i])
            else:
                assert bits32(got[i]) == bits32(want[i]), (route, i)
    batch = vb.lookup_messages_by_embeddings(qs[:65], 20, 0.5, accept_ordinals=messages.tolist())
    assert [bits32(x) for x in batch] == [bits32(vb.lookup_messages_by_embedding(q, 20, 0.5, accept_ordinals=messages.tolist())) for q in qs[:65]]
