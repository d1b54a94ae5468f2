"""CPU suite: the top-k distinct message lookups (`VectorBase.lookup_top_messages_by_embedding(s)`, `adapters.lookup_top_messages`) -- the
CPU twin of tests/test_gpu_top_messages.py over the same table, tests/top_messages_cases.py.

  1. the table covers every value of every axis, and its generators do what their names say;
  2. the table's two expected answers agree on the reference's own arithmetic: the numpy collapse of the reference's row hits (answer A's
     recipe) is `memory_messages_from_hits` + cut (answer B) up to the order among equal scores, and `judge_b` accepts it;
  3. the class's fallback path -- the all-survivor lookup and the collapse on the host -- on the engine doubles, single and a device group:
     every case equals the table's collapse, ordinals and float32 scores; batch == loop of single calls; K = 0 and K beyond 16384 answer;
  4. `adapters.lookup_top_messages`, the argument errors, and that header, option table and binding agree on the new names."""

from __future__ import annotations

import os
import re

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import top_messages_cases as tc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def single(monkeypatch, v, dtype="float32"):
    monkeypatch.setattr(_native, "Engine", FakeEngine)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    return vb


def group(monkeypatch, v, dtype="float32"):
    import torch

    from typeagent_py_amd.multidevice import DeviceGroup

    monkeypatch.setattr(_native, "Engine", FakeEngine)
    monkeypatch.setattr(DeviceGroup, "_topk_lists", lambda self, shards, nq, k: torch.zeros((shards, nq, k), dtype=torch.int64))
    monkeypatch.setattr(DeviceGroup, "_device_queries", lambda self, shards, a: [torch.from_numpy(a) for _ in shards])
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 1, 2], corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    return vb


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


def want_bits(case, qi, k=None):
    """The table's collapse of the reference's row hits, as (message, float32 score bits)."""
    hits = tc.reference_hits(case, qi)
    rm = tc.message_map(case.corpus.rows, case.map)
    m, s = tc.collapse([r for r, _ in hits], [sc for _, sc in hits], rm, tc.case_k(case) if k is None else k)
    return list(zip(m.tolist(), s.view(np.uint32).tolist()))


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_every_axis():
    assert {c.corpus.rows for c in tc.CASES} == set(tc.ROWS) and {c.corpus.dim for c in tc.CASES} == set(tc.WIDTHS)
    assert {c.corpus.dtype for c in tc.CASES} == {"float16", "float32"}
    for dim in tc.WIDTHS:
        assert {c.corpus.dtype for c in tc.CASES if c.corpus.dim == dim} == {"float16", "float32"}, dim
    assert {c.map for c in tc.CASES} == set(tc.MAPS) and {c.nq for c in tc.CASES} == set(tc.QUERIES)
    assert {c.k for c in tc.CASES} == set(tc.KS) and {c.thresholds for c in tc.CASES} == set(tc.THRESHOLDS)
    assert {c.allowed for c in tc.CASES} == set(tc.ALLOWED)
    assert len({c.name for c in tc.CASES}) == len(tc.CASES) and len(tc.B_CASES) == len(tc.CORPORA)
    # the single-query tier at 1536 with and without a row list, and a second pass (nine queries) with and without one
    wide1 = [c for c in tc.CASES if c.corpus.dim == 1536 and c.nq == 1]
    assert any(c.allowed == "none" for c in wide1) and any(c.allowed in ("random10", "range", "message_mask") for c in wide1)
    nine = [c for c in tc.CASES if c.nq == 9]
    assert any(c.allowed == "none" for c in nine) and any(c.allowed in ("random10", "range", "message_mask") for c in nine)


def test_the_generators_do_what_they_say():
    for rows in tc.ROWS:
        own, one, ch, il, holes, sparse = (tc.message_map(rows, k) for k in tc.MAPS)
        assert len(set(own.tolist())) == rows and set(one.tolist()) == {0}
        assert np.all(np.diff(ch) >= 0) and np.bincount(ch).max() <= 3
        if rows >= 64:
            assert np.any(np.diff(il) < 0)  # not monotone
            assert (holes == -1).sum() == rows // 5 and holes.max() == ch[holes >= 0].max()
            assert sparse.max() + 1 > 2 * len(set(sparse.tolist()))  # n_messages far beyond the messages in use
    for c in tc.CORPORA:
        v, held, qs = tc.corpus_arrays(c)
        assert v.shape == (c.rows, c.dim) and qs.shape == (tc.MAX_QUERIES, c.dim)
        if c.rows >= 63:
            assert np.isnan(v[c.rows // 3]).all() and not v[c.rows // 2].any() and np.isnan(v).any(axis=1).sum() == 1
            with np.errstate(invalid="ignore"):
                s = vo.scores_full(held, qs[0])
            assert s[c.rows // 2] == np.float32(0.5) and np.isnan(s[c.rows // 3])
            share = np.mean(s[~np.isnan(s)] >= np.float32(tc.tenth_threshold(c)))
            assert 0.05 <= share <= 0.15, (c.name, share)
    for case in tc.CASES:
        mask = tc.case_mask(case)
        if case.allowed == "empty":
            assert not mask.any()
        elif case.allowed == "random10" and case.corpus.rows >= 1000:
            assert 0.05 <= mask.mean() <= 0.15
        elif case.allowed == "range" and case.corpus.rows > 1:
            r = np.flatnonzero(mask)
            assert len(r) and np.all(np.diff(r) == 1)
    v, q = tc.tie_corpus()
    assert v.shape == (tc.TIE_ROWS, tc.TIE_DIM) and (v == v[0]).all() and tc.TIE_ROWS > tc.TIE_K > tc.TIE_BOUNDARY_KEYS


# ---- 2. A's recipe and B agree on the reference's arithmetic -------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_collapse_of_the_reference_hits_is_answer_b(case):
    for qi in range(case.nq):
        want = want_bits(case, qi)
        b = tc.expected_b(case, qi)
        k = tc.case_k(case)
        full = tc.mo.memory_messages_from_hits(tc.reference_hits(case, qi), tc.message_map(case.corpus.rows, case.map))
        # B before its cut, re-ordered by (score, ordinal), IS the collapse; B's own cut holds the same scores rank by rank
        resorted = sorted(((m, int(np.float32(s).view(np.uint32))) for m, s in full), key=lambda t: (-t[1], t[0]))
        assert resorted[:k] == want, (case.name, qi)
        assert [s for _, s in want] == [int(np.float32(s).view(np.uint32)) for _, s in b], (case.name, qi)
        n_pass = len(full)
        assert len(want) == min(k, n_pass)
        rep = tc.judge_b(case, qi, [m for m, _ in want], [float(np.uint32(s).view(np.float32)) for _, s in want])
        assert rep.k_returned == len(want)


# ---- 3. the fallback on the engine doubles ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.CASES, ids=[c.name for c in tc.CASES])
def test_fallback_equals_the_table(monkeypatch, case):
    v, held, qs = tc.corpus_arrays(case.corpus)
    vb = single(monkeypatch, v, case.corpus.dtype)
    rm = tc.message_map(case.corpus.rows, case.map)
    vb.set_row_messages(rm)
    mask = tc.case_mask(case)
    allowed = None if mask is None else (vb.message_mask(tc.allowed_messages(case)) if case.allowed == "message_mask" else mask)
    thr = tc.case_thresholds(case)
    with np.errstate(invalid="ignore"):
        got = vb.lookup_top_messages_by_embeddings(qs[: case.nq], tc.case_k(case), thr, allowed)
        assert len(got) == case.nq
        for qi in range(case.nq):
            assert bits32(got[qi]) == want_bits(case, qi), (case.name, qi)
            assert all(isinstance(h, ScoredInt) and isinstance(h.item, int) and isinstance(h.score, float) for h in got[qi])
        one = vb.lookup_top_messages_by_embedding(qs[0], tc.case_k(case), tc.threshold_of(case, 0), allowed)
    assert bits32(one) == bits32(got[0])
    assert not FakeEngine.instances[-1].options.get("top_messages")  # (a double has no such option: nothing was switched)


@pytest.mark.parametrize("builder", [single, group], ids=["single", "group"])
def test_fallback_k_outside_the_native_range_and_defaults(monkeypatch, builder):
    case = tc.Case(tc.CORPORA[6], "holes", 3, 10, "zero", "none")
    v, held, qs = tc.corpus_arrays(case.corpus)
    vb = builder(monkeypatch, v, case.corpus.dtype)
    vb.set_row_messages(tc.message_map(case.corpus.rows, case.map))
    probe = tc.Case(case.corpus, case.map, 3, 10, "zero", "none")
    with np.errstate(invalid="ignore"):
        for k, cut in ((0, 0), (16385, 16385), (None, 10), (7, 7)):
            got = vb.lookup_top_messages_by_embeddings(qs[:3], k, 0.0)
            for qi in range(3):
                assert bits32(got[qi]) == want_bits(probe, qi, cut), (k, qi)
        assert len(got[0]) == 7
        with pytest.raises(ValueError, match="max_hits must be >= 0"):
            vb.lookup_top_messages_by_embedding(qs[0], -1)
        assert vb.lookup_top_messages_by_embeddings(qs[:0], 5) == []


def test_the_lookup_this_call_exists_for(monkeypatch):
    v, q, rm = tc.motive_corpus()
    vb = single(monkeypatch, v)
    vb.set_row_messages(rm)
    rows = vb.lookup_messages_by_embedding(q, 5)
    top = vb.lookup_top_messages_by_embedding(q, 5)
    assert len(rows) < 5 and len(top) == 5
    assert top[0].item == rows[0].item == tc.MOTIVE_NEAR and np.float32(top[0].score) == np.float32(rows[0].score)
    assert len({h.item for h in top}) == 5 and all(a.score >= b.score for a, b in zip(top, top[1:]))


# ---- 4. the adapter, the errors, the names ----------------------------------------------------------------------------------------------

def test_adapter_and_errors(monkeypatch):
    case = tc.Case(tc.CORPORA[6], "interleaved", 2, 10, "zero", "message_mask")
    v, held, qs = tc.corpus_arrays(case.corpus)
    rm = tc.message_map(case.corpus.rows, case.map)
    vb = single(monkeypatch, v)
    with pytest.raises(RuntimeError, match="set_row_messages"):
        vb.lookup_top_messages_by_embedding(qs[0], 5)
    scope = tc.allowed_messages(case)
    with np.errstate(invalid="ignore"):
        got = adapters.lookup_top_messages(vb, qs[:2], rm, 10, 0.0, scope=scope.tolist())
        assert [bits32(g) for g in got] == [want_bits(case, 0), want_bits(case, 1)]
        handle = vb.message_mask(scope)
        assert isinstance(handle, RowMask)
        assert bits32(adapters.lookup_top_messages(vb, qs[0], rm, 10, 0.0, scope=handle)) == want_bits(case, 0)
        whole = tc.Case(case.corpus, case.map, 1, 10, "zero", "none")
        assert bits32(adapters.lookup_top_messages(vb, qs[0], rm, 10)) == want_bits(whole, 0)
    with pytest.raises(TypeError, match="sequence"):
        adapters.lookup_top_messages(vb, qs[0], lambda r: 0, 10)
    with pytest.raises(ValueError, match="1D embedding or a 2D"):
        adapters.lookup_top_messages(vb, qs[None, :2], rm, 10)
    # a mask built before the index changed is refused as elsewhere
    vb.remove_rows([0])
    with pytest.raises(ValueError, match="build it again|covers"):
        vb.lookup_top_messages_by_embedding(qs[0], 5, 0.0, handle)
    other = single(monkeypatch, v)
    other.set_row_messages(rm)
    with pytest.raises(ValueError, match="another index"):
        vb.lookup_top_messages_by_embedding(qs[0], 5, 0.0, other.message_mask([1, 2]))


def test_header_option_table_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    csrc = os.path.join(ROOT, "typeagent_py_amd", "csrc")
    abi, ctx = open(os.path.join(csrc, "tavb_abi.hip")).read(), open(os.path.join(csrc, "tavb_ctx.h")).read()
    assert int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1)) == _native.ABI_VERSION == 7
    for name in ("tavb_search_top_messages", "tavb_search_top_messages_device"):
        assert name in _native.ABI_SYMBOLS and re.search(rf"\bint {name}\(", header)
    assert 'SWITCH("top_messages", top_messages)' in abi and re.search(r"int64_t top_messages = 1;", ctx) and '"top_messages"' in header
    body = ctx[ctx.index("void for_each_buffer(F&& f) {"):]
    assert re.search(r"^\s*Buffer d_msg_best;", ctx, re.M) and "&d_msg_best" in body[: body.index("\n  }\n")]
    assert hasattr(_native.Engine, "search_top_messages") and hasattr(_native.Engine, "search_top_messages_device")
