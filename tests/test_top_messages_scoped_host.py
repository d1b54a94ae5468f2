"""CPU suite: the scoped top-k distinct message lookups (`VectorBase.lookup_top_messages_by_embeddings_scoped`,
`adapters.lookup_top_messages_in_scopes`, tavb_search_top_messages_scoped) without a GPU -- the CPU twin of
tests/test_gpu_top_messages_scoped.py over the same table, tests/top_messages_scoped_cases.py.

  1. the table covers every value of every axis and each of the hand-added cases, and its generators do what their names say;
  2. the device route restated in numpy -- per pass of eight queries the union list, `scoped_batch_cases.member_bytes`, and the
     `ScopedMessageMaxSink` (`sink_best`: max per (query, message) over the union positions whose bit is set), in sub-groups with
     bit0 > 0 as well -- gives, per case and query, what `top_messages_cases.collapse` gives over the query's own scope;
  3. the class on a recording engine double: identical handles delegate to the one-mask call, the rest is ONE scoped call with
     identical handles adjacent, no slot for an empty scope and the answers in the caller's order; "top_messages_scoped" = 0,
     "top_messages" = 0, K = 0, K = 16385 and a handle without a device mask loop over the one-mask call;
  4. argument errors, the adapter, and that header, option table, binding and built library agree on the new names."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_batch_cases as sc
from tests import top_messages_scoped_cases as ts
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("tavb_search_top_messages_scoped", "tavb_search_top_messages_scoped_device")


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def reference_scores(case, qi):
    """float32 scores of every row for query qi, by the reference's arithmetic; NaN rows stay NaN (they never pass)."""
    _, held, _ = ts.corpus_arrays(case.corpus)
    with np.errstate(invalid="ignore"):
        return vo.scores_full(held, ts.case_queries(case)[qi]).astype(np.float32)


def want_bits(case, qi, scope=None, k=None):
    """`collapse` over the passing rows of query qi's own scope, as (message, float32 score bits)."""
    scope = ts.case_scopes(case)[qi] if scope is None else scope
    s = reference_scores(case, qi)
    with np.errstate(invalid="ignore"):
        rows = np.flatnonzero(scope & (s >= vo.f32_threshold(ts.threshold_of(case, qi))))
    m, best = ts.collapse(rows, s[rows], ts.message_map(case.corpus.rows, case.map), ts.case_k(case) if k is None else k)
    return list(zip(m.tolist(), best.view(np.uint32).tolist()))


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_every_axis_and_every_hand_added_case():
    cases = ts.CASES
    assert {c.corpus.rows for c in cases} == set(ts.ROWS) == set(sc.ROWS) and {c.corpus.dim for c in cases} == set(ts.WIDTHS)
    assert {c.corpus.dtype for c in cases if c.corpus.dim == 72} == {"float16"}
    for dim in (6, 8, 1536):
        assert {c.corpus.dtype for c in cases if c.corpus.dim == dim} == {"float16", "float32"}, dim
    shuffled = [c for c in cases if not c.note]
    assert {c.map for c in shuffled} == set(ts.MAPS) and {c.nq for c in shuffled} == set(ts.BATCHES) == {1, 2, 8, 9, 17}
    assert {c.k for c in shuffled} == set(ts.KS) and {c.thresholds for c in shuffled} == set(ts.THRESHOLDS)
    assert {c.family for c in shuffled} == set(ts.FAMILIES) == set(sc.FAMILIES) and {c.form for c in shuffled} == {"raw", "handles"}
    assert {c.form for c in cases} == set(ts.FORMS)
    assert len({c.name for c in cases}) == len(cases) == 66 + len(ts.HAND)
    assert len(ts.B_CASES) == len(ts.CORPORA) - 1 and all(ts.expect_native(c) for c in ts.B_CASES)
    native = sum(ts.expect_native(c) for c in cases)
    assert 40 <= native < len(cases)  # both sides of `expect_native` are well populated
    h = ts.HAND
    # 1. interleaved x disjoint at 8 and 9 queries: every message has chunks in several queries' scopes
    for c in (h["1a"], h["1b"]):
        rm, scopes = ts.message_map(c.corpus.rows, c.map), ts.case_scopes(c)
        assert c.map == "interleaved" and c.family == "disjoint" and ts.expect_native(c)
        for m in range(ts.n_messages(c)):
            assert sum(bool(s[rm == m].any()) for s in scopes) >= 2, (c.name, m)
    assert (h["1a"].nq, h["1b"].nq) == (8, 9)
    # 2. one message, disjoint scopes
    assert h["2"].map == "one" and h["2"].family == "disjoint" and ts.n_messages(h["2"]) == 1
    # 3. nine queries at 4099 x 1536 fp16, nested; at the floor one query's slots already fill "topk_scores_bytes": sub-groups of one
    c = h["3"]
    assert (c.corpus.rows, c.corpus.dim, c.corpus.dtype, c.nq, c.family) == (4099, 1536, "float16", 9, "nested")
    assert ts.FLOOR_BYTES // (ts.n_messages(c) * 4) <= 1
    # 4. 129 queries over five distinct masks: 17 passes, one more than a wave holds
    c = h["4"]
    assert (c.corpus.rows, c.corpus.dim, c.nq) == (33, 8, 129) and len({id(s) for s in ts.case_scopes(c)}) == 5 and len(ts.passes(c.nq)) == 17
    # 5. the adopted corpus; 6. the forms
    assert ts.ORDINAL_BASE == 1_000_003 and h["5"].note.endswith("adopted")
    assert [h[x].form for x in ("6a", "6b", "6c", "6d")] == ["raw", "handles", "message_handles", "host_only"]
    assert not ts.expect_native(h["6d"]) and ts.expect_native(h["6c"])
    kinds = [kind for kind, _ in ts.scope_specs(h["6c"])]
    assert "messages" in kinds and "ranges" in kinds


def test_the_generators_do_what_they_say():
    for c in ts.CASES:
        scopes = ts.case_scopes(c)
        assert len(scopes) == c.nq and all(s.dtype == np.bool_ and s.shape == (c.corpus.rows,) for s in scopes), c.name
        fam = c.family
        if fam == "identical":
            assert all(s is scopes[0] for s in scopes) and not ts.expect_native(c)
        elif fam == "disjoint":
            assert np.sum(scopes, axis=0).max() == 1 and np.logical_or.reduce(scopes).all()
        elif fam == "nested":
            assert all((a <= b).all() for a, b in zip(scopes, scopes[1:]))
        elif fam == "one_empty":
            assert sum(not s.any() for s in scopes) == 1
        elif fam == "first_row":
            assert np.flatnonzero(scopes[c.nq // 2]).tolist() == [0]
        elif fam == "last_row":
            assert np.flatnonzero(scopes[c.nq // 2]).tolist() == [c.corpus.rows - 1]
        elif fam == "all_rows":
            assert all(s.all() for s in scopes) and len({id(s) for s in scopes}) == c.nq
        elif fam == "all_empty":
            assert not any(s.any() for s in scopes) and not ts.expect_native(c)
        thr = ts.case_thresholds(c)
        assert (isinstance(thr, list) and len(thr) == c.nq) if c.thresholds == "per_query" else isinstance(thr, float)
        assert ts.case_queries(c).shape == (c.nq, c.corpus.dim)
    for corpus in ts.CORPORA:  # the parent table's judge sees the same first nine queries
        np.testing.assert_array_equal(ts.corpus_arrays(corpus)[2][: ts.tc.MAX_QUERIES], ts.tc.corpus_arrays(corpus)[2])
    assert ts.passes(9) == [8, 1] and ts.passes(17) == [8, 8, 1] and ts.passes(2) == [2]


# ---- 2. the device route in numpy ----------------------------------------------------------------------------------------------------------

def decoded(best_row: np.ndarray, k: int):
    """One query's slots -> (message, score bits), what launch_message_hist and the selection leave: slot - 1, by (-score, message), cut at k."""
    msgs = np.flatnonzero(best_row)
    bits = best_row[msgs] - np.uint32(1)
    order = np.lexsort((msgs, -bits.view(np.float32).astype(np.float64)))[:k]
    return list(zip(msgs[order].tolist(), bits[order].tolist()))


@pytest.mark.parametrize("case", ts.CASES, ids=[c.name for c in ts.CASES])
def test_membership_bytes_and_the_sink_give_the_collapse_over_the_own_scope(case):
    scopes, rm, n_msgs, k = ts.case_scopes(case), ts.message_map(case.corpus.rows, case.map), ts.n_messages(case), ts.case_k(case)
    scores = np.stack([reference_scores(case, qi) for qi in range(min(case.nq, ts.MAX_QUERIES))])
    q0 = 0
    for n in ts.passes(case.nq):
        masks = scopes[q0: q0 + n]
        rows = np.flatnonzero(np.logical_or.reduce(masks))  # the ascending union list of the pass
        member = sc.member_bytes(masks, rows)
        s = scores[(q0 + np.arange(n)) % ts.MAX_QUERIES][:, rows]
        with np.errstate(invalid="ignore"):
            passing = np.stack([s[j] >= vo.f32_threshold(ts.threshold_of(case, q0 + j)) for j in range(n)])
        whole = ts.sink_best(member, 0, n, s, passing, rm[rows], n_msgs)
        for sub in (1, 3):  # sub-groups of the pass: bit0 > 0
            for s0 in range(0, n, sub):
                m = min(sub, n - s0)
                part = ts.sink_best(member, s0, m, s[s0: s0 + m], passing[s0: s0 + m], rm[rows], n_msgs)
                np.testing.assert_array_equal(part, whole[s0: s0 + m])
        for j in range(n):
            assert decoded(whole[j], k) == want_bits(case, q0 + j), (case.name, q0 + j)
        q0 += n
    # a shared message is scored per scope: under disjoint scopes over one message every query has its own single score
    if case.map == "one" and case.family == "disjoint":
        firsts = [want_bits(case, qi) for qi in range(case.nq)]
        assert all(len(f) == 1 and f[0][0] == 0 for f in firsts) and len({f[0][1] for f in firsts}) > 1


# ---- 3. the class on a recording double ----------------------------------------------------------------------------------------------------

class RecordingEngine(FakeEngine):
    """The engine double with what a single-GPU engine needs for the masked and top-messages routes: torch CPU tensors stand in for device
    memory, the two options default to 1 as on the device, and every top-messages call is recorded."""

    def __init__(self, device=None, use_torch_stream=False):
        super().__init__(device, use_torch_stream)
        self.calls: list = []
        self.options.update(top_messages=1, top_messages_scoped=1)

    def mask_to_rows(self, mask):
        return self.mask_to_rows_bits(mask)[:2]

    def mask_to_rows_bits(self, mask):
        import torch

        m = np.asarray(mask, dtype=bool)
        flat = np.flatnonzero(m)
        return torch.from_numpy(flat.astype(np.int32)), len(flat), torch.from_numpy(_native.pack_mask_bits(m).view(np.int32).copy())

    def _rows_of(self, dev_bits):
        return np.flatnonzero(np.unpackbits(dev_bits.numpy().view(np.uint8), bitorder="little")[: self.rows]).astype(np.int64)

    def search_subset_batch_resident(self, queries, dev_rows, k, thrs, remap=True):
        raise AssertionError("a top-messages lookup has no business on the row lookups of this double")

    def _top(self, queries, row_lists, k, thrs):
        nq = len(queries)
        t = np.broadcast_to(np.asarray(thrs, dtype=np.float32), (nq,))
        msgs, scs, cnts = np.zeros((nq, k), np.int64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        for i, q in enumerate(queries):
            rows = row_lists[i]
            with np.errstate(invalid="ignore"):
                s = vo.cosine_to_score(np.dot(self.corpus[rows], np.asarray(q, dtype=np.float32))).astype(np.float32)
                ok = s >= t[i]
            m, best = ts.collapse(rows[ok], s[ok], self.row_messages, k)
            msgs[i, : len(m)], scs[i, : len(m)], cnts[i] = m, best, len(m)
        return msgs, scs, cnts

    def search_top_messages(self, queries, k, thrs, dev_rows=None):
        assert 1 <= k <= _native.MAX_LARGE_K
        self.calls.append(("one_mask", len(queries)))
        rows = np.arange(self.rows, dtype=np.int64) if dev_rows is None else dev_rows.numpy().astype(np.int64)
        return self._top(queries, [rows] * len(queries), k, thrs)

    def search_top_messages_scoped(self, queries, dev_bits_list, k, thrs):
        dev_bits_list = list(dev_bits_list)
        assert 1 <= k <= _native.MAX_LARGE_K and len(dev_bits_list) == len(queries) and queries.flags.c_contiguous
        assert np.asarray(thrs).shape == (len(queries),) and np.asarray(thrs).dtype == np.float32
        self.calls.append(("scoped", [b.data_ptr() for b in dev_bits_list], np.array(queries), np.array(thrs)))
        return self._top(queries, [self._rows_of(b) for b in dev_bits_list], k, thrs)


N, D = 300, 24


@pytest.fixture(scope="module")
def corpus():
    from tests.synth import make_corpus, make_queries

    v, _ = make_corpus(N, D, 9760)
    return v, make_queries(9, D, 9761), ts.message_map(N, "interleaved")


def build(monkeypatch, v, rm=None, engine=RecordingEngine):
    monkeypatch.setattr(_native, "Engine", engine)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb.add_embeddings(None, v)
    if rm is not None:
        vb.set_row_messages(rm)
    return vb


def some_masks(n, seed=9763):
    rng = np.random.default_rng(seed)
    return {"a": rng.random(n) < 0.5, "b": rng.random(n) < 0.2, "c": np.arange(n) % 3 == 0, "empty": np.zeros(n, dtype=bool)}


def test_grouping_caller_order_and_empty_scopes(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v, rm)
    eng = vb.engine
    masks = some_masks(N)
    h = {name: vb.row_mask(m) for name, m in masks.items()}
    assert h["empty"].count == 0 and all(x.dev_bits is not None for x in h.values())
    order = ["a", "b", "empty", "a", "c", "b", "a", "empty", "c"]
    thr = [0.0, 0.45, 0.0, 0.5, None, 0.4, 0.55, 0.0, 1.5]
    got = vb.lookup_top_messages_by_embeddings_scoped(qs, [h[name] for name in order], 7, thr)
    assert [c[0] for c in eng.calls] == ["scoped"]
    _, ptrs, sent, sent_thr = eng.calls[0]
    name_of = {h[name].dev_bits.data_ptr(): name for name in masks}
    assert [name_of[p] for p in ptrs] == ["a", "a", "a", "b", "b", "c", "c"]  # equal handles adjacent, groups by first query, no empty scope
    np.testing.assert_array_equal(sent, qs[[0, 3, 6, 1, 5, 4, 8]])
    np.testing.assert_array_equal(sent_thr, np.asarray([0.0, 0.5, 0.55, 0.45, 0.4, 0.0, 1.5], dtype=np.float32))
    eng.calls.clear()
    for i, name in enumerate(order):  # ... and the answers in the caller's order: the definition, query by query
        want = vb.lookup_top_messages_by_embedding(qs[i], 7, thr[i], h[name])
        assert bits32(got[i]) == bits32(want), (i, name)
        assert all(isinstance(x, ScoredInt) and isinstance(x.item, int) and isinstance(x.score, float) for x in got[i])
    assert got[2] == [] and got[7] == [] and got[8] == [] and len(got[0]) == 7
    assert {c[0] for c in eng.calls} == {"one_mask"}
    # a message with chunks in two scopes is scored per scope: "interleaved" puts every message into both halves
    lo, hi = np.arange(N) < N // 2, np.arange(N) >= N // 2
    two = vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [lo, hi], N, 0.0)
    both = vb.lookup_top_messages_by_embeddings_scoped(np.stack([qs[0], qs[0]]), [lo, hi], N, 0.0)
    assert {x.item for x in both[0]} == {x.item for x in both[1]} and bits32(both[0]) != bits32(both[1]) and bits32(two[0]) == bits32(both[0])
    # raw arrays: each object one scope, an object that repeats resolved once
    eng.calls.clear()
    got2 = vb.lookup_top_messages_by_embeddings_scoped(qs[:4], [masks["a"], masks["b"], masks["a"], masks["b"]], 5, 0.0)
    assert [c[0] for c in eng.calls] == ["scoped"] and len(set(eng.calls[0][1])) == 2 and eng.calls[0][1][0] == eng.calls[0][1][1]
    assert [bits32(x) for x in got2] == [bits32(vb.lookup_top_messages_by_embedding(qs[i], 5, 0.0, masks["ab"[i % 2]])) for i in range(4)]
    # every scope empty (distinct handles), or no query: no call at all
    eng.calls.clear()
    assert vb.lookup_top_messages_by_embeddings_scoped(qs[:3], [np.zeros(N, dtype=bool) for _ in range(3)], 7) == [[], [], []]
    assert vb.lookup_top_messages_by_embeddings_scoped(qs[:0], [], 7) == []
    assert eng.calls == []


def test_identical_handles_delegate_to_the_one_mask_call(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v, rm)
    eng = vb.engine
    h = vb.row_mask(some_masks(N)["a"])
    got = vb.lookup_top_messages_by_embeddings_scoped(qs[:5], [h] * 5, 10, [0.0, 0.5, 0.4, 1.5, None])
    assert eng.calls == [("one_mask", 5)]
    want = vb.lookup_top_messages_by_embeddings(qs[:5], 10, [0.0, 0.5, 0.4, 1.5, None], h)
    assert [bits32(x) for x in got] == [bits32(x) for x in want] and got[3] == []
    eng.calls.clear()
    raw = some_masks(N)["b"]
    vb.lookup_top_messages_by_embeddings_scoped(qs[:5], [raw] * 5, 10)
    vb.lookup_top_messages_by_embeddings_scoped(qs[:1], [h])
    assert eng.calls == [("one_mask", 5), ("one_mask", 1)]


@pytest.mark.parametrize("why", ["top_messages_scoped=0", "top_messages=0", "k=0", "k=16385", "host_only", "no_call", "group"])
def test_everything_else_loops_over_the_one_mask_call(monkeypatch, corpus, why):
    v, qs, rm = corpus
    if why == "group":
        import torch

        from typeagent_py_amd.multidevice import DeviceGroup

        monkeypatch.setattr(_native, "Engine", FakeEngine)
        monkeypatch.setattr(DeviceGroup, "_topk_lists", lambda self, shards, nq, k: torch.zeros((shards, nq, k), dtype=torch.int64))
        monkeypatch.setattr(DeviceGroup, "_device_queries", lambda self, shards, a: [torch.from_numpy(a) for _ in shards])
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 1, 2])
        vb.add_embeddings(None, v)
        vb.set_row_messages(rm)
    else:
        vb = build(monkeypatch, v, rm, FakeEngine if why == "no_call" else RecordingEngine)
    eng = vb.engine
    masks = some_masks(N)
    names = ("a", "b", "empty", "c")
    h = [vb.row_mask(masks[name]) for name in names]
    k = {"k=0": 0, "k=16385": _native.MAX_LARGE_K + 1}.get(why, 6)
    if "=" in why and not why.startswith("k"):
        eng.set_option(why.split("=")[0], 0)
    if why == "host_only":
        h[1].dev_bits = None
    thr = [0.45, 0.0, 0.0, None]
    got = vb.lookup_top_messages_by_embeddings_scoped(qs[:4], h, k, thr)
    calls = getattr(eng, "calls", [])
    assert not any(c[0] == "scoped" for c in calls)
    if why in ("top_messages_scoped=0", "host_only"):
        assert calls == [("one_mask", 1)] * 3  # (the empty scope answers without a call)
    for i, name in enumerate(names):
        probe = ts.Case(ts.Corpus(N, D, "float32", 0), "interleaved", 4, k, "zero", "identical")
        s = vo.scores_full(v, qs[i]).astype(np.float32)
        rows = np.flatnonzero(masks[name] & (s >= vo.f32_threshold(0.0 if thr[i] is None else thr[i])))
        m, best = ts.collapse(rows, s[rows], rm, k)
        assert probe.k == k and [x.item for x in got[i]] == m.tolist(), (why, i)
        np.testing.assert_allclose([x.score for x in got[i]], best, atol=1e-6, rtol=0)
        assert bits32(got[i]) == bits32(vb.lookup_top_messages_by_embedding(qs[i], k, thr[i], h[i])), (why, i)
    assert got[2] == [] and len(got[1]) == (6 if k == 6 else len(set(rm[masks["b"]].tolist())))


def test_argument_errors(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v)
    masks = some_masks(N)
    a, b = vb.row_mask(masks["a"]), vb.row_mask(masks["b"])
    with pytest.raises(RuntimeError, match="set_row_messages"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b])
    vb.set_row_messages(rm[:-1])
    with pytest.raises(ValueError, match=f"covers {N - 1} rows, the index has {N}"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b])
    vb.set_row_messages(rm)
    with pytest.raises(ValueError, match="Number of scopes 1 does not match number of embeddings 2"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a])
    with pytest.raises(ValueError, match="2D"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[0], [a])
    with pytest.raises(ValueError, match="Number of thresholds"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], 5, [0.1])
    with pytest.raises(ValueError, match="max_hits must be >= 0"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, b], -1)
    with pytest.raises(TypeError, match="must be bool"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, np.zeros(N, dtype=np.int64)])
    with pytest.raises(ValueError, match=f"covers 5 rows, the index has {N}"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, np.zeros(5, dtype=bool)])
    other = build(monkeypatch, v, rm)
    with pytest.raises(ValueError, match="another index"):
        vb.lookup_top_messages_by_embeddings_scoped(qs[:2], [a, other.row_mask(masks["b"])])
    # a stale handle: rows were removed, then the length restored
    fresh, half = other.row_mask(np.ones(N, dtype=bool)), other.row_mask(masks["a"])
    other.remove_rows([0])
    other.add_embeddings(None, v[:1])
    other.set_row_messages(rm)
    with pytest.raises(ValueError, match="build it again"):
        other.lookup_top_messages_by_embeddings_scoped(qs[:2], [fresh, half])


# ---- 4. the adapter and the names ------------------------------------------------------------------------------------------------------------

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


def test_the_adapter_makes_one_mask_per_distinct_scope_object(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = build(monkeypatch, v)
    eng = vb.engine
    when = _Scope([_Collection([_Range((5, 0), (30, 0))]), _Collection([_Range((10, 0), (50, 0)), _Range((2, 0))])])
    col = _Collection([_Range((40, 0), (55, 0))])
    msgs = [3, 4, 5, 17, 58]
    made = []
    real = adapters._scope_mask
    monkeypatch.setattr(adapters, "_scope_mask", lambda vector_base, scope: made.append(id(scope)) or real(vector_base, scope))
    handle = None
    scopes = [msgs, when, col, msgs, when, [when, col], msgs]
    got = adapters.lookup_top_messages_in_scopes(vb, qs[:7], rm, scopes, 4, 0.3)
    assert made == [id(msgs), id(when), id(col), id(scopes[5])]  # one mask per distinct object, in the order of first use
    assert [c[0] for c in eng.calls] == ["scoped"] and len(set(eng.calls[0][1])) == 3  # ([when, col] is empty and takes no slot)
    monkeypatch.setattr(adapters, "_scope_mask", real)
    for i, scope in enumerate(scopes):
        assert bits32(got[i]) == bits32(adapters.lookup_top_messages(vb, qs[i], rm, 4, 0.3, scope=scope)), i
    assert got[1] and {x.item for x in got[1]} <= set(range(10, 30)) and got[5] == [] and len(got[0]) == 4
    handle = vb.message_mask(msgs)
    assert isinstance(handle, RowMask)
    again = adapters.lookup_top_messages_in_scopes(vb, qs[:2], rm, [handle, col], 4, [0.3, 0.3])
    assert bits32(again[0]) == bits32(got[0]) and bits32(again[1]) == bits32(adapters.lookup_top_messages(vb, qs[1], rm, 4, 0.3, scope=col))
    assert adapters.lookup_top_messages_in_scopes(vb, qs[:0], rm, []) == []
    with pytest.raises(TypeError, match="row_to_message as a sequence"):
        adapters.lookup_top_messages_in_scopes(vb, qs[:1], lambda r: 0, [msgs])
    with pytest.raises(ValueError, match="Number of scopes 1 does not match"):
        adapters.lookup_top_messages_in_scopes(vb, qs[:2], rm, [msgs])
    with pytest.raises(ValueError, match="2D"):
        adapters.lookup_top_messages_in_scopes(vb, qs[0], rm, [msgs])
    assert "lookup_top_messages_in_scopes" in adapters.lookup_top_messages.__doc__


def test_header_option_table_binding_and_library_agree():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    csrc = os.path.join(ROOT, "typeagent_py_amd", "csrc")
    abi, ctx = open(os.path.join(csrc, "tavb_abi.hip")).read(), open(os.path.join(csrc, "tavb_ctx.h")).read()
    lib = _native.load_library()
    assert lib.tavb_version() == _native.ABI_VERSION == 7 == int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1))
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    assert 'SWITCH("top_messages_scoped", top_messages_scoped)' in abi and re.search(r"int64_t top_messages_scoped = 1;", ctx)
    assert '"top_messages_scoped"' in header and re.search(r"9 = a scoped top-messages batch", header)
    for method in ("search_top_messages_scoped", "search_top_messages_scoped_device"):
        assert callable(getattr(_native.Engine, method))
    # without a GPU there is no context: both calls refuse that first, with a message, and write nothing
    q, thr = np.zeros((2, 4), dtype=np.float32), np.zeros(2, dtype=np.float32)
    out = np.full((2, 3), 7, dtype=np.int64)
    a = _native._addr
    assert lib.tavb_search_top_messages_scoped(None, a(q), 2, None, 10, 3, a(thr), a(out), None, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_top_messages_scoped_device(None, a(q), 2, None, 10, 3, a(thr), a(out)) == -1 and b"null context" in lib.tavb_last_error()
    assert out.min() == 7
