"""CPU suite: the scoped message lookups without a GPU -- the case table of tests/message_scope_cases.py pinned against numpy (the twin of
`mask_from_messages_kernel` against np.isin), `VectorBase.message_mask` / `lookup_messages_by_embedding(s)_masked` /
`lookup_messages_by_embeddings` / `adapters.lookup_messages_in_scope` on the engine double and on a device group of doubles against the
compositions they are defined as and against oracle/messages_oracle.py, their argument errors, and the C ABI's additive symbols."""

import os
import re

import numpy as np
import pytest

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests import message_scope_cases as sc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, ScoredInt, TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 240, 32
NEW_SYMBOLS = ("tavb_mask_from_messages", "tavb_search_messages_masked", "tavb_search_messages_batch")


# ---- the table itself ------------------------------------------------------------------------------------------------------------------

def test_the_mask_table_covers_what_it_claims():
    assert {c.rows for c in sc.MASK_CASES} == set(sc.MASK_ROWS) and {c.n_messages for c in sc.MASK_CASES} == set(sc.MASK_MESSAGES)
    assert {c.layout for c in sc.MASK_CASES} == {"contiguous", "interleaved"} and len(sc.MASK_CASES) == 96
    longer = holes = 0
    for case in sc.MASK_CASES:
        m = sc.mask_case_map(case)
        assert len(m) >= case.rows and m.min() >= -1 and m.max() < case.n_messages
        live = m[m >= 0]
        if len(live):
            assert np.bincount(live).max() <= 5  # messages of 1 to 5 chunks
        longer += len(m) > case.rows
        holes += bool((m[: case.rows] < 0).any())
        sets = sc.accept_sets(case.n_messages, case.seed)
        assert list(sets) == ["empty", "every", "first", "last", "duplicates", "out_of_range"]
        assert len(sets["duplicates"]) > len(set(sets["duplicates"].tolist()))
        assert (sets["out_of_range"] < 0).any() and (sets["out_of_range"] >= case.n_messages).any()
    assert longer >= 20 and holes >= 60
    big = sc.mask_case_map(next(c for c in sc.MASK_CASES if c.rows == 4097 and c.n_messages == 700 and c.layout == "contiguous"))
    assert all((np.diff(np.flatnonzero(big == msg)) <= 5).all() for msg in (3, 300, 650))  # contiguous: a message's chunks lie together


@pytest.mark.parametrize("case", sc.MASK_CASES, ids=[c.name for c in sc.MASK_CASES])
def test_the_kernel_twin_equals_isin(case):
    m = sc.mask_case_map(case)
    n_bits = int(m.max()) + 1 if (m >= 0).any() else 0
    for name, accept in sc.accept_sets(case.n_messages, case.seed).items():
        want = sc.isin_mask(m, case.rows, accept)
        words = sc.twin_mask_words(m, case.rows, accept, n_bits)
        assert words.dtype == np.uint32 and words.shape == ((case.rows + 31) // 32,)
        np.testing.assert_array_equal(words, _native.pack_mask_bits(want), err_msg=f"{case.name} {name}")
        if name == "every":
            assert want.sum() == (m[: case.rows] >= 0).sum()
        if name == "empty":
            assert not words.any()


def test_the_lookup_table_covers_what_it_claims():
    cases = sc.LOOKUP_CASES
    assert len(cases) == len(sc.CORPORA) * len(sc.ROUTES) * len(sc.SHAPES)
    for corpus in sc.CORPORA:
        for route in sc.ROUTES:
            mine = [c for c in cases if c.corpus == corpus and c.route == route]
            assert {c.nq for c in mine} == {1, 8, 9, 33, 64, 65, 130}
            assert {c.max_matches for c in mine} == {1, 10, 64, 65, 256, None}
            assert {c.scope for c in mine} == {"0%", "1%", "50%", "100%", "rows"}
            assert {c.thresholds for c in mine} == {"uniform", "per_query"}
    m = sc.lookup_map()
    assert m.shape == (sc.ROWS,) and m.max() == sc.N_MESSAGES - 1 and 100 < (m < 0).sum() < 600 and np.bincount(m[m >= 0]).max() <= 5
    assert len(sc.scope_messages("1%")) == 10 and len(sc.scope_messages("50%")) == 500 and len(sc.scope_messages("0%")) == 0
    rows = sc.arbitrary_rows_mask()
    assert (m[rows] < 0).any() and 1000 < rows.sum() < 1400
    # what the forced routes serve, against the planners the class asks (the rule with no floors: yes exactly when the route serves the shape)
    for corpus in sc.CORPORA:
        dt = _native.TAVB_F16 if corpus.dtype == "float16" else _native.TAVB_F32
        for k in (1, 10, 64, 65, 256):
            assert sc.tile_serves(corpus, k) == (k <= 64 and _native.plan_masked(64, k, corpus.dim, dt, 1, 1, 0, 0))
            assert sc.wide_serves(corpus, k) == _native.plan_masked_wide(_native.MFMA_MIN_BATCH, k, corpus.dim, dt, 1, 1, 0, 0)
    routes = {(c.corpus.name, c.route, c.max_matches): sc.expected_route(c) for c in cases}
    assert routes[("fp16-d72", "tile", 10)] == 1 and routes[("fp16-d64", "tile", 65)] == 1 and routes[("fp16-d64", "tile", 64)] == 2
    assert routes[("fp32-d64", "wide", 10)] == 1 and routes[("fp16-d72", "wide", 256)] == 3 and routes[("fp32-d64", "tile", 1)] == 2


# ---- the class on the doubles ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 9700)
    return v, make_queries(6, D, 9701), sc.message_map(70, N, "interleaved", 9702)


def single(monkeypatch, v):
    monkeypatch.setattr(_native, "Engine", FakeEngine)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb.add_embeddings(None, v)
    return vb


def group(monkeypatch, v):
    import torch

    from typeagent_py_amd.multidevice import DeviceGroup

    monkeypatch.setattr(_native, "Engine", FakeEngine)
    monkeypatch.setattr(DeviceGroup, "_topk_lists", lambda self, shards, nq, k: torch.zeros((shards, nq, k), dtype=torch.int64))
    monkeypatch.setattr(DeviceGroup, "_device_queries", lambda self, shards, a: [torch.from_numpy(a) for _ in shards])
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 1, 2])
    vb.add_embeddings(None, v)
    return vb


BUILDERS = {"double": single, "group": group}


def scopes(row_messages):
    n_msg = int(row_messages.max()) + 1
    rng = np.random.default_rng(9703)
    return {
        "none": [],
        "one": [int(row_messages[row_messages >= 0][5])],
        "half": rng.choice(n_msg, n_msg // 2, replace=False).tolist(),
        "all": list(range(n_msg)),
        "noisy": [-3, n_msg, n_msg + 9, 4, 4, 11, 2**40],
    }


def pairs(hits):
    assert all(isinstance(h, ScoredInt) for h in hits)
    return [(h.item, h.score) for h in hits]


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_message_mask_is_the_isin_mask(monkeypatch, corpus, kind):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    vb.set_row_messages(np.concatenate([rm, [5, 6, 7]]))  # a map longer than the index
    for name, scope in scopes(rm).items():
        want = sc.isin_mask(rm, N, np.asarray(scope, dtype=np.int64))
        for given in (scope, np.asarray(scope, dtype=np.int64), set(scope), iter(scope)):
            handle = vb.message_mask(given)
            assert isinstance(handle, RowMask) and handle.rows == N and handle.count == int(want.sum()), name
            np.testing.assert_array_equal(handle.flat(), np.flatnonzero(want))
        np.testing.assert_array_equal(vb.row_mask(want).flat(), vb.message_mask(scope).flat())
    assert not (rm[vb.message_mask(scopes(rm)["all"]).flat()] < 0).any()


@pytest.mark.parametrize("kind", list(BUILDERS))
@pytest.mark.parametrize("max_matches", [None, 1, 10, 300, 0])
def test_masked_message_lookups_equal_their_composition(monkeypatch, corpus, kind, max_matches):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    vb.set_row_messages(rm)
    per_query = [0.0, 0.5, 0.45, 0.55, 1.5, 0.4]
    rows_mask = np.random.default_rng(9704).random(N) < 0.5  # arbitrary rows, some without a message
    assert (rm[rows_mask] < 0).any()
    allowed = {name: vb.message_mask(scope) for name, scope in scopes(rm).items()}
    allowed["rows"] = vb.row_mask(rows_mask)
    allowed["raw"] = rows_mask
    for name, mask in allowed.items():
        flat = (np.flatnonzero(mask) if name == "raw" else mask.flat()).tolist()
        for thr in (None, 0.5, per_query):
            got = vb.lookup_messages_by_embeddings_masked(qs, mask, max_matches, thr)
            assert len(got) == len(qs)
            for i, q in enumerate(qs):
                t = thr[i] if isinstance(thr, list) else thr
                want = vb.lookup_messages_in_subset_by_embedding(q, flat, max_matches, t)
                assert pairs(got[i]) == pairs(want), (name, i, thr)
                if not isinstance(thr, list):
                    assert pairs(vb.lookup_messages_by_embedding_masked(q, mask, max_matches, t)) == pairs(want)
                # the memory provider's semantics over the same rows (oracle): best score per message, sorted
                ref = mo.memory_lookup_in_subset_by_embedding(lambda e, rows, k, ms: vo.lookup_in_subset(v, e, rows, k, ms), q,
                                                              np.where(rm < 0, 10**6, rm), flat, max_matches, t)
                ref = [(m, s) for m, s in ref if m != 10**6]
                assert [m for m, _ in pairs(got[i])] == [m for m, _ in ref], (name, i, thr)
                np.testing.assert_allclose([s for _, s in pairs(got[i])], [s for _, s in ref], atol=1e-6, rtol=0)
    assert vb.lookup_messages_by_embeddings_masked(qs[:0], allowed["half"], max_matches) == []
    assert vb.lookup_messages_by_embeddings_masked(qs, allowed["none"], max_matches) == [[] for _ in qs]


@pytest.mark.parametrize("kind", list(BUILDERS))
@pytest.mark.parametrize("max_matches", [None, 1, 10, 300])
def test_batched_message_lookups_equal_the_single_calls(monkeypatch, corpus, kind, max_matches):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    vb.set_row_messages(rm)
    per_query = [0.0, 0.5, 0.45, 0.55, 1.5, 0.4]
    for accept in (None, scopes(rm)["half"], scopes(rm)["noisy"], []):
        for thr in (None, 0.5, per_query):
            got = vb.lookup_messages_by_embeddings(qs, max_matches, thr, accept_ordinals=None if accept is None else iter(accept))
            for i, q in enumerate(qs):
                t = thr[i] if isinstance(thr, list) else thr
                assert pairs(got[i]) == pairs(vb.lookup_messages_by_embedding(q, max_matches, t, accept_ordinals=accept))
                # the sqlite provider's semantics (oracle): top-k over the whole corpus, THEN the filter
                ref = mo.sqlite_lookup_by_embedding(lambda e, k, ms: vo.lookup(v, e, k, ms), q, rm.tolist(), max_matches, t, accept)
                assert [m for m, _ in pairs(got[i])] == [m for m, _ in ref]
                np.testing.assert_allclose([s for _, s in pairs(got[i])], [s for _, s in ref], atol=1e-6, rtol=0)
    assert vb.lookup_messages_by_embeddings(qs[:0], max_matches) == []


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_lookup_messages_in_scope(monkeypatch, corpus, kind):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    scope = scopes(rm)["half"]
    flat = np.flatnonzero(sc.isin_mask(rm, N, np.asarray(scope))).tolist()
    for max_matches in (None, 3, 10):
        for thr in (None, 0.5):
            want = [adapters.lookup_messages_in_subset(vb, q, flat, rm, max_matches, thr) for q in qs]
            assert [pairs(x) for x in adapters.lookup_messages_in_scope(vb, qs, rm, scope, max_matches, thr)] == [pairs(x) for x in want]
            assert pairs(adapters.lookup_messages_in_scope(vb, qs[2], rm, set(scope), max_matches, thr)) == pairs(want[2])
            handle = vb.message_mask(scope)
            assert pairs(adapters.lookup_messages_in_scope(vb, qs[1], rm, handle, max_matches, thr)) == pairs(want[1])
            if max_matches is not None:
                assert all(len(x) <= max_matches for x in want)
    # a narrow scope is SEARCHED: the post-filter of the sqlite form finds nothing where the best chunks lie outside it
    far = [int(m) for m in np.unique(rm[rm >= 0]) if m not in {h.item for h in vb.lookup_messages_by_embedding(qs[0], 10)}][:3]
    assert vb.lookup_messages_by_embedding(qs[0], 10, accept_ordinals=far) == []
    assert sorted(h.item for h in adapters.lookup_messages_in_scope(vb, qs[0], rm, far, 10)) == sorted(far)
    with pytest.raises(TypeError, match="sequence"):
        adapters.lookup_messages_in_scope(vb, qs[0], lambda row: 0, scope)
    with pytest.raises(ValueError, match="1D embedding or a 2D"):
        adapters.lookup_messages_in_scope(vb, qs[None], rm, scope)


def test_argument_errors(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = single(monkeypatch, v)
    mask = np.ones(N, dtype=bool)
    for call in (lambda: vb.message_mask([1, 2]), lambda: vb.lookup_messages_by_embeddings_masked(qs, mask),
                 lambda: vb.lookup_messages_by_embedding_masked(qs[0], mask), lambda: vb.lookup_messages_by_embeddings(qs)):
        with pytest.raises(RuntimeError, match="set_row_messages"):  # no map set
            call()
    vb.set_row_messages(rm[: N - 1])  # a map that is too short
    for call in (lambda: vb.message_mask([1, 2]), lambda: vb.lookup_messages_by_embeddings_masked(qs, mask), lambda: vb.lookup_messages_by_embeddings(qs)):
        with pytest.raises(ValueError, match="covers 239 rows, the index has 240"):
            call()
    vb.set_row_messages(rm)
    other = single(monkeypatch, v)
    other.set_row_messages(rm)
    with pytest.raises(ValueError, match="another index"):
        vb.lookup_messages_by_embeddings_masked(qs, other.message_mask([1, 2]))
    stale = vb.message_mask([1, 2])
    vb.add_embeddings(None, v[:1])
    vb.set_row_messages(np.concatenate([rm, [0]]))
    with pytest.raises(ValueError, match="mask covers 240 rows, the index has 241"):
        vb.lookup_messages_by_embeddings_masked(qs, stale)
    fresh = vb.message_mask([1, 2])
    for call in (lambda: vb.lookup_messages_by_embeddings_masked(qs, fresh, 10, [0.5] * 5), lambda: vb.lookup_messages_by_embeddings(qs, 10, [0.5] * 7)):
        with pytest.raises(ValueError, match="Number of thresholds"):
            call()
    with pytest.raises(ValueError, match="Expected 2D"):
        vb.lookup_messages_by_embeddings_masked(qs[0], fresh)
    with pytest.raises(ValueError, match="Expected 1D"):
        vb.lookup_messages_by_embedding_masked(qs, fresh)
    with pytest.raises(ValueError, match="Expected 2D"):
        vb.lookup_messages_by_embeddings(qs[0])
    with pytest.raises(TypeError, match="integers"):
        vb.message_mask([0.5, 1.5])
    with pytest.raises(ValueError, match="max_hits must be >= 0"):
        vb.lookup_messages_by_embeddings_masked(qs, fresh, -1)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_the_abi_is_additive():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1)) == 7 == _native.ABI_VERSION
    assert int(re.search(r"#define TAVB_KERNEL_COUNT (\d+)", header).group(1)) == 10
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _native.load_library(preload_torch=False)
    assert lib.tavb_version() == 7
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(tavb_ctx\* ctx,", code), f"{name} is not declared in include/tavb.h"
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    # without a context every new entry point fails cleanly
    assert lib.tavb_mask_from_messages(None, None, 0, 0, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_messages_batch(None, None, 0, 1, None, None, -1, 1, None, None, None) == -1
    assert lib.tavb_search_messages_masked(None, None, 0, None, 0, 0, 0, None, 0, 1, None, 1, 1, None, None, None) == -1
    for method in ("mask_from_messages", "search_messages_masked", "search_messages_batch"):
        assert callable(getattr(_native.Engine, method))
    for method in ("message_mask", "lookup_messages_by_embedding_masked", "lookup_messages_by_embeddings_masked", "lookup_messages_by_embeddings"):
        assert callable(getattr(VectorBase, method))
