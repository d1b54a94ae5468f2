"""GPU suite: scoped batches -- one row mask per query in a single submission (tavb_search_scoped_batch / _device,
tavb_search_messages_scoped, the `ScopedSelector` of the streaming scan and `scope_member_kernel`) under
`VectorBase.fuzzy_lookup_embeddings_scoped`, `lookup_messages_by_embeddings_scoped` and `adapters.lookup_messages_in_scopes`.  The table is
tests/scoped_batch_cases.py; tests/test_scoped_batch_host.py pins it on the CPU.

  1. every case: the batch equals the per-query `fuzzy_lookup_embedding_in_subset` over np.flatnonzero(scope) on the same index bit for
     bit -- ordinals, float32 score bits, counts; no near-tie allowance, both sides are the streaming kernels' arithmetic -- and passes
     the standing parity definition against the CPU oracle (`check_topk_parity` with the float64 referee, scores within 1e-5);
     `masked_route` is 4 where the native route ran and 1 where identical handles went to the one-scope call;
  2. the membership bytes equal their numpy twin on the mask-tail row counts, over masks with dirty tails, the bytes behind untouched;
  3. the C calls themselves: a word behind each output buffer stays untouched, the device twin's keys equal the synchronous call's, and
     bad arguments come back as errors with a message;
  4. the message forms equal the per-query message calls bit for bit on a map with rows mapped to -1, with a TextRangesInScope per query;
  5. an adopted corpus with ordinal_base != 0.
"""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import mask_algebra_cases as mc
from tests import scoped_batch_cases as sc
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

pytestmark = pytest.mark.gpu

_state: dict = {}


def _torch():
    import torch

    return torch


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def rows_of(corpus: sc.Corpus):
    """(the corpus' MAX_ROWS rows, the same rows as the device holds them, MAX_QUERIES queries), made once."""
    if corpus.name not in _state:
        v, _ = make_corpus(sc.MAX_ROWS, corpus.dim, corpus.seed)
        held = v.astype(np.float16).astype(np.float32) if corpus.dtype == "float16" else v
        _state[corpus.name] = (v, held, make_queries(sc.MAX_QUERIES, corpus.dim, corpus.seed + 1))
    return _state[corpus.name]


def index(corpus: sc.Corpus, rows: int):
    """The index over the first `rows` rows of the corpus, built once."""
    key = (corpus.name, rows)
    if key not in _state:
        v, held, qs = rows_of(corpus)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=corpus.dtype)
        vb.add_embeddings(None, v[:rows])
        _state[key] = (vb, held[:rows], qs)
    return _state[key]


def shared_handles(vb, scopes):
    """One RowMask per distinct array object: queries that share a scope share the handle."""
    made: dict = {}
    for s in scopes:
        if id(s) not in made:
            made[id(s)] = vb.row_mask(s)
    return [made[id(s)] for s in scopes]


def scope_arguments(vb, case: sc.Case, scopes):
    """The scopes as the case hands them over: RowMask handles or the arrays themselves."""
    return shared_handles(vb, scopes) if case.as_handles else scopes


def check_against_subset_and_oracle(vb, held, qs, scopes, thr, k, got, what):
    for i, scope in enumerate(scopes):
        flat = np.flatnonzero(scope)
        t = thr[i] if isinstance(thr, list) else thr
        want = vb.fuzzy_lookup_embedding_in_subset(qs[i], flat, k, t)
        assert bits32(got[i]) == bits32(want), (what, i)
        if len(flat) == 0:
            assert got[i] == []
            continue
        sub = held[flat]
        vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [h.item for h in got[i]], [h.score for h in got[i]], k, 0.0 if t is None else t,
                             candidate_ordinals=flat, referee=vo.f64_referee(sub, qs[i]))


# ---- 1. every case through the class -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", sc.CASES, ids=[c.name for c in sc.CASES])
def test_case(case):
    vb, held, qs = index(case.corpus, case.rows)
    eng = vb.engine
    scopes = sc.case_scopes(case)
    thr = sc.case_thresholds(case)
    args = scope_arguments(vb, case, scopes)
    native = sc.expect_native(scopes)
    if native:  # a one-scope lookup first, so that the 4 below is this call's
        vb.fuzzy_lookup_embeddings_masked(qs[:1], np.ones(case.rows, dtype=bool), 1)
        assert eng.get_option("masked_route") == 1
    before = eng.get_option("masked_route")
    got = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], args, case.max_hits, thr)
    assert len(got) == case.nq
    if native:
        assert eng.get_option("masked_route") == 4
        assert eng.get_option("last_tier") == case.corpus.tier  # the vector tier for aligned rows (a one-query pass at 1536 too), else the scalar tier
    elif len({id(s) for s in scopes}) == 1 and scopes[0].any():
        assert eng.get_option("masked_route") == 1  # one scope for all (or one query): the one-scope call, on the row list
    else:
        assert eng.get_option("masked_route") == before  # nothing to search: no call
        assert got == [[] for _ in range(case.nq)]
    check_against_subset_and_oracle(vb, held, qs, scopes, thr, case.max_hits, got, case.name)
    o, s, c = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], args, case.max_hits, thr, as_arrays=True)
    assert o.shape == s.shape == (case.nq, case.max_hits) and c.tolist() == [len(x) for x in got]
    for i in range(case.nq):
        assert list(zip(o[i, : c[i]].tolist(), s[i, : c[i]].view(np.uint32).tolist())) == bits32(got[i])


# ---- 2. the membership bytes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", sc.ROWS)
def test_membership_bytes_equal_the_numpy_twin(rows):
    torch = _torch()
    eng = _native.Engine(0)
    eng.set_corpus_tensor(torch.zeros((rows, 8), dtype=torch.float32, device="cuda"))
    rng = np.random.default_rng(9870 + rows)
    masks = [rng.random(rows) < p for p in (0.5, 0.1, 0.9, 0.5, 0.02, 0.5, 0.7, 0.3)]
    masks[2][-1] = True  # the last row, whose word has the dirty tail
    masks[0][0] = masks[1][0] = True  # row 0; no union below is empty
    # packed with every bit at or beyond `rows` set and a word of ones behind: the kernel reads no bit it should not
    dev = [torch.from_numpy(mc.pack(m, dirty=True).view(np.int32).copy()).cuda() for m in masks]
    for n_masks in (1, 3, 8):
        union = np.flatnonzero(np.logical_or.reduce(masks[:n_masks])).astype(np.int32)
        want = sc.member_bytes(masks[:n_masks], union)
        assert want.min() >= 1
        dev_rows = torch.from_numpy(union).cuda()
        got = eng.mask_membership(dev[:n_masks], dev_rows)
        eng.synchronize()
        np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f"rows {rows}, {n_masks} masks")
        # the library itself, with bytes behind the output
        raw = torch.full((len(union) + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        ptrs = (ctypes.c_void_p * n_masks)(*[m.data_ptr() for m in dev[:n_masks]])
        torch.cuda.synchronize()
        rc = eng.lib.tavb_mask_membership(eng._h, ptrs, n_masks, rows, ctypes.c_void_p(dev_rows.data_ptr()), len(union), ctypes.c_void_p(raw.data_ptr()))
        assert rc == 0, eng.lib.tavb_last_error()
        eng.synchronize()
        out = raw.cpu().numpy()
        np.testing.assert_array_equal(out[: len(union)], want)
        assert (out[len(union):] == 0xAB).all(), "bytes behind the membership bytes were written"
    # every row, in any order: rows no mask holds give 0
    every = torch.from_numpy(np.arange(rows, dtype=np.int32)[::-1].copy()).cuda()
    got = eng.mask_membership(dev, every)
    eng.synchronize()
    np.testing.assert_array_equal(got.cpu().numpy(), sc.member_bytes(masks, np.arange(rows)[::-1]))
    eng.close()


# ---- 3. the C calls --------------------------------------------------------------------------------------------------------------------------

TWIN_CASES = [c for i, c in enumerate(sc.CASES) if i % 4 == 1 and sc.expect_native(sc.case_scopes(c))]


@pytest.mark.parametrize("case", TWIN_CASES, ids=[c.name for c in TWIN_CASES])
def test_guard_words_and_the_device_twin(case):
    torch = _torch()
    vb, held, qs = index(case.corpus, case.rows)
    eng = vb.engine
    nq, k = case.nq, case.max_hits
    scopes = sc.case_scopes(case)
    handles = shared_handles(vb, scopes)
    bits = [h.dev_bits for h in handles]  # (empty scopes included: the library gives them empty lists)
    thr = sc.case_thresholds(case)
    t = np.ascontiguousarray(np.broadcast_to(np.asarray([_native.f32_threshold(0.0 if x is None else x) for x in thr] if isinstance(thr, list) else
                                                        _native.f32_threshold(thr), dtype=np.float32), (nq,)))
    q = np.ascontiguousarray(qs[:nq])
    # the synchronous call over buffers with one more element behind them
    ords, scs, cnts = np.full(nq * k + 1, -77, dtype=np.int64), np.full(nq * k + 1, -77.0, dtype=np.float32), np.full(nq + 1, -77, dtype=np.int32)
    ptrs = (ctypes.c_void_p * nq)(*[b.data_ptr() for b in bits])
    a = _native._addr
    rc = eng.lib.tavb_search_scoped_batch(eng._h, a(q), nq, ptrs, case.rows, k, a(t), a(ords), a(scs), a(cnts))
    assert rc == 0, eng.lib.tavb_last_error()
    assert ords[-1] == -77 and scs[-1] == -77.0 and cnts[-1] == -77, "an element behind an output buffer was written"
    assert eng.get_option("masked_route") == 4
    ords, scs, cnts = ords[:-1].reshape(nq, k), scs[:-1].reshape(nq, k), cnts[:-1]
    for i, scope in enumerate(scopes):
        want = vb.fuzzy_lookup_embedding_in_subset(qs[i], np.flatnonzero(scope), k, thr[i] if isinstance(thr, list) else thr)
        assert list(zip(ords[i, : cnts[i]].tolist(), scs[i, : cnts[i]].view(np.uint32).tolist())) == bits32(want), (case.name, i)
    # the device twin: keys behind which one more key stays untouched, equal to the synchronous call's
    out = torch.full((nq * k + 1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_scoped_device(torch.from_numpy(q).cuda(), bits, k, t, out_keys=out)
    eng.synchronize()
    keys = out.cpu().numpy()
    assert keys[-1] == 0x5A5A5A5A5A5A5A5A, "the key behind the device twin's output was written"
    o2, s2, c2 = _native.decode_keys(keys[:-1].view(np.uint64).reshape(nq, k))
    assert c2.tolist() == cnts.tolist()
    for i in range(nq):
        assert o2[i, : c2[i]].tolist() == ords[i, : cnts[i]].tolist() and s2[i, : c2[i]].view(np.uint32).tolist() == scs[i, : cnts[i]].view(np.uint32).tolist()
    # ... and into pinned host memory
    pinned = torch.zeros((nq, k), dtype=torch.int64).pin_memory()
    eng.search_scoped_device(torch.from_numpy(q).cuda(), bits, k, t, out_keys=pinned)
    eng.synchronize()
    np.testing.assert_array_equal(pinned.numpy().reshape(-1), keys[:-1])


def test_argument_errors_on_the_device():
    torch = _torch()
    vb, _, qs = index(sc.CORPORA[0], 1000)
    eng = vb.engine
    lib, a = eng.lib, _native._addr
    h = vb.row_mask(np.arange(1000) % 2 == 0)
    q = np.ascontiguousarray(qs[:2])
    t = np.zeros(2, dtype=np.float32)
    ords, scs, cnts = np.zeros((2, 300), dtype=np.int64), np.zeros((2, 300), dtype=np.float32), np.full(2, 9, dtype=np.int32)
    good = (ctypes.c_void_p * 2)(h.dev_bits.data_ptr(), h.dev_bits.data_ptr())
    holed = (ctypes.c_void_p * 2)(h.dev_bits.data_ptr(), None)

    def sync(masks=good, rows=1000, k=5, queries=a(q), out=a(ords)):
        return lib.tavb_search_scoped_batch(eng._h, queries, 2, masks, rows, k, a(t), out, a(scs), a(cnts))

    assert sync() == 0 and cnts.tolist() == [5, 5]
    for kwargs, text in (({"k": 0}, b"k must be >= 1"), ({"k": 257}, b"1 <= k <= 256"), ({"rows": 999}, b"the mask covers 999 rows, the corpus has 1000"),
                         ({"masks": None}, b"null dev_masks"), ({"masks": holed}, b"the mask of query 1 is null"), ({"queries": None}, b"null argument"),
                         ({"out": None}, b"null argument")):
        assert sync(**kwargs) == -1 and text in lib.tavb_last_error(), (kwargs, lib.tavb_last_error())
    dq = torch.from_numpy(q).cuda()
    keys = torch.zeros((2, 5), dtype=torch.int64, device="cuda")
    assert lib.tavb_search_scoped_device(eng._h, ctypes.c_void_p(dq.data_ptr()), 2, holed, 1000, 5, a(t), ctypes.c_void_p(keys.data_ptr())) == -1
    assert b"the mask of query 1 is null" in lib.tavb_last_error()
    assert lib.tavb_search_scoped_device(eng._h, ctypes.c_void_p(dq.data_ptr()), 2, good, 1000, 5, a(t), None) == -1 and b"null argument" in lib.tavb_last_error()
    assert lib.tavb_search_messages_scoped(eng._h, a(q), 2, good, 1000, 5, a(t), 5, a(ords), a(scs), a(cnts)) == -3  # no row -> message map
    assert b"message map" in lib.tavb_last_error()
    # no query: nothing happens, whatever the other arguments
    assert lib.tavb_search_scoped_batch(eng._h, None, 0, None, 1000, 5, None, None, None, None) == 0
    with pytest.raises(ValueError, match="1 masks for 2 queries"):
        eng.search_scoped_batch(q, [h.dev_bits], 5, t)
    with pytest.raises(ValueError, match="1 <= k <= 256"):
        eng.search_scoped_batch(q, [h.dev_bits] * 2, 300, t)
    # the context still serves lookups
    assert sync() == 0 and cnts.tolist() == [5, 5]


# ---- 4. the message forms ----------------------------------------------------------------------------------------------------------------

class _Loc:
    def __init__(self, m, c=0):
        self.message_ordinal, self.chunk_ordinal = m, c


class _Range:
    def __init__(self, start, end=None):
        self.start, self.end = _Loc(*start), (None if end is None else _Loc(*end))


class _Collection:
    def __init__(self, ranges):
        self._ranges = ranges

    def get_ranges(self):
        return self._ranges


class _Scope:  # TextRangesInScope, duck-typed
    def __init__(self, text_ranges):
        self.text_ranges = text_ranges


@pytest.mark.parametrize("corpus", [sc.CORPORA[3], sc.CORPORA[5], sc.CORPORA[1]], ids=lambda c: c.name)
@pytest.mark.parametrize("max_matches", [1, 10, 65, None])
def test_message_lookups_per_scope(corpus, max_matches):
    rows, n_messages = 1000, 300
    v, _, qs = rows_of(corpus)
    key = ("messages", corpus.name)
    if key not in _state:
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=corpus.dtype)
        vb.add_embeddings(None, v[:rows])
        rm = np.sort(np.random.default_rng(9880).integers(0, n_messages, rows))
        rm[np.random.default_rng(9881).random(rows) < 0.15] = -1  # rows without a message
        vb.set_row_messages(rm)
        _state[key] = (vb, rm)
    vb, rm = _state[key]
    eng = vb.engine
    rng = np.random.default_rng(9882)
    week = vb.range_mask([[(40, 120)]], of="messages")
    thread = vb.message_mask(rng.choice(n_messages, 60, replace=False))
    arbitrary = vb.row_mask(rng.random(rows) < 0.3)  # rows, some of them without a message
    assert (rm[arbitrary.flat()] < 0).any()
    nothing = vb.message_mask([])
    handles = [week, thread, week & thread, arbitrary, nothing, week | thread, thread, ~week, week - thread]
    thr = [0.0, 0.5, None, 0.45, 0.0, 0.55, 0.4, 1.5, 0.5]
    got = vb.lookup_messages_by_embeddings_scoped(qs[:9], handles, max_matches, thr)
    assert eng.get_option("masked_route") == 4
    for i, h in enumerate(handles):
        want = vb.lookup_messages_by_embedding_masked(qs[i], h, max_matches, thr[i])
        assert bits32(got[i]) == bits32(want), (corpus.name, max_matches, i)
        sub = vb.lookup_messages_in_subset_by_embedding(qs[i], h.flat().tolist(), max_matches, thr[i])
        assert bits32(got[i]) == bits32(sub), (corpus.name, max_matches, i)
    assert got[4] == [] and got[7] == [] and any(got[i] for i in (0, 1, 3, 5))
    # one TextRangesInScope (or another kind of scope) per query through the adapter
    scopes = [_Scope([_Collection([_Range((40, 0), (120, 0))])]),
              _Scope([_Collection([_Range((10, 0), (200, 0))]), _Collection([_Range((150, 0), (290, 0)), _Range((20, 0))])]),
              rng.choice(n_messages, 30, replace=False).tolist(), thread, _Collection([_Range((0, 0), (5, 0))]), _Scope(None)]
    scopes.append(scopes[0])  # the same object twice: one mask
    vb.fuzzy_lookup_embeddings_masked(qs[:1], arbitrary, 1)
    got = adapters.lookup_messages_in_scopes(vb, qs[:7], rm, scopes, max_matches, 0.45)
    assert eng.get_option("masked_route") == 4
    for i, scope in enumerate(scopes):
        assert bits32(got[i]) == bits32(adapters.lookup_messages_in_scope(vb, qs[i], rm, scope, max_matches, 0.45)), (corpus.name, max_matches, i)
    assert got[0] and all(40 <= x.item < 120 for x in got[0]) and all(150 <= x.item < 200 or x.item == 20 for x in got[1])


# ---- 5. an adopted corpus with an ordinal base ---------------------------------------------------------------------------------------------

def test_adopted_corpus_with_an_ordinal_base():
    torch = _torch()
    case = sc.ADOPTED
    _, held, qs = rows_of(case.corpus)
    held = held[: case.rows]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    vb.adopt_device_corpus(torch.from_numpy(held.astype(np.float16)).cuda(), ordinal_base=sc.ORDINAL_BASE)
    eng = vb.engine
    assert eng.ordinal_base == sc.ORDINAL_BASE
    scopes = sc.case_scopes(case)
    thr = sc.case_thresholds(case)
    handles = [vb.row_mask(s) for s in scopes]
    got = vb.fuzzy_lookup_embeddings_scoped(qs[: case.nq], handles, case.max_hits, thr)
    assert eng.get_option("masked_route") == 4
    check_against_subset_and_oracle(vb, held, qs, scopes, thr, case.max_hits, got, "adopted")
    # the engine's own ordinals, and the device twin's keys, carry the base
    t = np.asarray([_native.f32_threshold(0.0 if x is None else x) for x in thr], dtype=np.float32)
    o, s, c = eng.search_scoped_batch(qs[: case.nq], [h.dev_bits for h in handles], case.max_hits, t)
    keys = eng.search_scoped_device(torch.from_numpy(np.ascontiguousarray(qs[: case.nq])).cuda(), [h.dev_bits for h in handles], case.max_hits, t)
    eng.synchronize()
    o2, s2, c2 = _native.decode_keys(keys.cpu().numpy().view(np.uint64))
    for i in range(case.nq):
        assert (o[i, : c[i]] - sc.ORDINAL_BASE).tolist() == [h.item for h in got[i]] and c[i] == c2[i]
        assert o2[i, : c2[i]].tolist() == o[i, : c[i]].tolist() and s2[i, : c2[i]].view(np.uint32).tolist() == s[i, : c[i]].view(np.uint32).tolist()
    assert any(c) and int(o[c > 0][0, 0]) >= sc.ORDINAL_BASE


# ---- 6. widths whose eight queries do not fit the vector tier's LDS, and batches of several waves ------------------------------------------

@pytest.mark.parametrize("dtype,dim", [("float32", 4800), ("float16", 4808), ("float32", 9608)])
@pytest.mark.parametrize("max_hits", [10, 65])
def test_wide_rows_keep_the_single_query_arithmetic(dtype, dim, max_hits):
    """8 x dim x 4 bytes of queries exceed the vector tier's 150 KiB (4800: four per pass fit, 9608: two): the passes are cut to what fits,
    so that a pass runs on the vector tier as the single-query lookup does -- not on the scalar tier's element loop -- and the scores stay
    bit for bit."""
    rows, nq = 257, 9
    key = ("wide", dtype, dim)
    if key not in _state:
        v, _ = make_corpus(rows, dim, 9890)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
        vb.add_embeddings(None, v)
        _state[key] = (vb, v.astype(np.float16).astype(np.float32) if dtype == "float16" else v, make_queries(nq, dim, 9891))
    vb, held, qs = _state[key]
    rng = np.random.default_rng(9892)
    scopes = [rng.random(rows) < 0.5 for _ in range(nq)]
    thr = [sc.THR_CYCLE[i % len(sc.THR_CYCLE)] for i in range(nq)]
    got = vb.fuzzy_lookup_embeddings_scoped(qs, scopes, max_hits, thr)
    assert vb.engine.get_option("masked_route") == 4 and vb.engine.get_option("last_tier") == 2
    check_against_subset_and_oracle(vb, held, qs, scopes, thr, max_hits, got, key)


@pytest.mark.parametrize("max_hits", [10, 65])
def test_a_batch_of_several_waves(max_hits):
    """A wave is 16 passes -- 128 queries, 64 from max_hits 65 on: 131 queries are two waves, or three, the last of them short."""
    corpus, rows, nq = sc.CORPORA[0], 257, 131
    vb, held, _ = index(corpus, rows)
    qs = make_queries(nq, corpus.dim, 9893)
    rng = np.random.default_rng(9894)
    made = [rng.random(rows) < p for p in (0.5, 0.1, 0.9, 0.02, 0.0)]
    scopes = [made[int(j)] if j < len(made) else rng.random(rows) < 0.4 for j in rng.integers(0, 2 * len(made), nq)]
    thr = [sc.THR_CYCLE[i % len(sc.THR_CYCLE)] for i in range(nq)]
    got = vb.fuzzy_lookup_embeddings_scoped(qs, shared_handles(vb, scopes), max_hits, thr)
    assert vb.engine.get_option("masked_route") == 4
    check_against_subset_and_oracle(vb, held, qs, scopes, thr, max_hits, got, ("waves", max_hits))


def test_a_forced_scalar_tier_is_followed():
    """Option "force_tier" = 3 sends the single-query lookups to the scalar tier's element loop: a scoped pass goes with them."""
    corpus, rows, nq = sc.CORPORA[3], 1000, 9
    vb, held, qs = index(corpus, rows)
    eng = vb.engine
    rng = np.random.default_rng(9895)
    scopes = [rng.random(rows) < 0.5 for _ in range(nq)]
    eng.set_option("force_tier", 3)
    try:
        got = vb.fuzzy_lookup_embeddings_scoped(qs[:nq], scopes, 10, 0.0)
        assert eng.get_option("masked_route") == 4 and eng.get_option("last_tier") == 3
        check_against_subset_and_oracle(vb, held, qs, scopes, 0.0, 10, got, "forced scalar tier")
    finally:
        eng.set_option("force_tier", 0)
