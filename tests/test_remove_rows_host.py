"""CPU suite: removing rows without a GPU.  `VectorBase.remove_rows` / `remove_at` on an engine double whose `compact_rows` is np.delete,
against the verbatim reference class with `_vectors = np.delete(_vectors, which, axis=0)`; the bookkeeping around it (the mirror is not
uploaded again, the row -> message map, the subset cache, the removal epoch of `RowMask`, matrices somebody else holds, the device-group
fallback); the case table of tests/remove_rows_cases.py; `adapters.install_remove_term` over the reference's own consumers; and the C
ABI's additive symbol."""

import asyncio
import os
import re
import sqlite3

import numpy as np
import pytest

from oracle import ref_loader, ref_wrappers
from tests import remove_rows_cases as rc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel, create_test_embedding_model
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 300, 24
needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="the verbatim reference is only present in the build container")


class CompactingEngine(FakeEngine):
    """The engine double with the two calls `remove_rows` makes: the packed mask "uploaded" (counted), the corpus compacted by np.delete."""

    def mask_bits_to_device(self, words):
        self.mask_uploads = getattr(self, "mask_uploads", 0) + 1
        return np.array(words, dtype=np.uint32)

    def compact_rows(self, dev_remove_bits):
        flags = np.unpackbits(np.asarray(dev_remove_bits, dtype="<u4").view(np.uint8), bitorder="little")[: self.rows].astype(bool)
        kept = np.delete(self.corpus[: self.rows], np.flatnonzero(flags), axis=0)
        self.corpus[: len(kept)] = kept
        self.rows = len(kept)
        self.compactions = getattr(self, "compactions", 0) + 1
        return self.rows


@pytest.fixture
def fake(monkeypatch):
    from typeagent_py_amd import multidevice

    monkeypatch.setattr(_native, "Engine", CompactingEngine)
    monkeypatch.setattr(multidevice._native, "Engine", CompactingEngine)


def new_vb(v=None, **kw) -> VectorBase:
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), **kw)
    if v is not None:
        vb.add_embeddings(None, np.array(v, dtype=np.float32))
    return vb


def pairs(res):
    return [(r.item, r.score) for r in res]


def same(a, b):
    assert [r.item for r in a] == [r.item for r in b]
    np.testing.assert_allclose([r.score for r in a], [r.score for r in b], atol=1e-6, rtol=0)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_what_it_claims():
    cases = rc.cases()
    assert rc.CHUNK == _native.MASK_ROWS_PER_WORKGROUP and rc.CHUNK % rc.ODD_PASS != 0 and rc.ODD_PASS % rc.TILE == 0
    assert 120 <= len(cases) <= 200 and len({c.id for c in cases}) == len(cases)
    assert {c.rows for c in cases} == set(rc.ROWS) == {1, 2, 31, 32, 33, 64, 16383, 16384, 16385, 2 * 16384 + 17}
    assert {(c.dim, c.dtype) for c in cases} == set(rc.SMALL_SHAPES + rc.WIDE_SHAPES + rc.NARROW_SHAPES)
    assert {c.rows for c in cases if c.dim in (384, 1536)} == set(rc.AROUND_CHUNK)
    assert {c.kind for c in cases} == set(rc.KINDS) and {c.route for c in cases} == set(rc.ROUTES)
    assert {c.pass_rows for c in cases if c.route == "in_place"} >= {0, 64, rc.CHUNK, rc.ODD_PASS}
    assert all(c.pass_rows == 0 for c in cases if c.route == "out_of_place")
    for rows in rc.ROWS:  # every kind that exists at a size is in the table at that size
        for kind in rc.KINDS:
            if kind != "block_longer_than_pass" and rc.removed_flags(kind, rows, 64) is not None:
                assert any(c.rows == rows and c.kind == kind for c in cases), (rows, kind)
    for route in rc.ROUTES:
        assert {c.kind for c in cases if c.route == route} >= set(rc.KINDS) - {"block_longer_than_pass"}
    many = [c for c in cases if c.route == "in_place" and c.rows > 4 * rc.effective_pass(c.pass_rows, c.dim, c.dtype)]
    assert len(many) >= 10  # many passes
    for c in cases:
        f = rc.flags(c)
        assert f.shape == (c.rows,) and f.dtype == np.bool_
        m = rc.matrix(c)
        assert m.shape == (c.rows, c.dim) and np.array_equal(m.astype(np.float16).astype(np.float32), m)
        p = rc.effective_pass(c.pass_rows, c.dim, c.dtype)
        assert p % rc.TILE == 0 and p >= rc.TILE
        if c.kind == "none":
            assert not f.any()
        elif c.kind == "all":
            assert f.all()
        elif c.kind == "all_but_first":
            assert not f[0] and f[1:].all()
        elif c.kind == "all_but_last":
            assert not f[-1] and f[:-1].all()
        elif c.kind == "every_other":
            assert f.sum() == c.rows // 2 and not f[0]
        elif c.kind == "block_in_chunk":
            i = np.flatnonzero(f)
            assert len(i) and i[-1] - i[0] + 1 == len(i) and i[0] // rc.CHUNK == i[-1] // rc.CHUNK
        elif c.kind == "block_over_chunk_edge":
            i = np.flatnonzero(f)
            assert i[-1] - i[0] + 1 == len(i) and i[0] < rc.CHUNK <= i[-1]
        elif c.kind == "block_longer_than_pass":
            i = np.flatnonzero(f)
            assert i[-1] - i[0] + 1 == len(i) > p and c.route == "in_place" and 0 < i[0] and i[-1] < c.rows - 1
        elif c.kind.startswith("random"):
            assert f.sum() == max(1, c.rows * int(c.kind.split("_")[1]) // 100)
    for dim in (8, 100, 384, 1536, 33):
        m = rc.base_matrix(dim)
        assert len(np.unique(m[:, :2], axis=0)) == len(m)  # no two rows alike: a misplaced row shows


def test_the_twin_of_the_passes_equals_np_delete():
    """The in-place algorithm as the library runs it -- passes of whole tiles from the tile of the first removed row on, every pass
    gathered into a staging array and written back at the count of kept rows before it -- restated in numpy over the table."""
    for c in rc.cases():
        if c.route != "in_place" or c.dim > 100:
            continue
        f = rc.flags(c)
        a = np.arange(c.rows)
        want = np.delete(a, np.flatnonzero(f))
        if f.any():
            p = rc.effective_pass(c.pass_rows, c.dim, c.dtype)
            first = int(np.argmax(f))
            for r0 in range(first // rc.TILE * rc.TILE, c.rows, p):
                r1 = min(r0 + p, c.rows)
                staged = a[r0:r1][~f[r0:r1]].copy()
                dst = int((~f[:r0]).sum())
                assert dst + len(staged) <= r1  # the write ends at or below the end of the pass: later passes read only beyond it
                a[dst : dst + len(staged)] = staged
        np.testing.assert_array_equal(a[: len(want)], want, err_msg=c.id)


# ---- the class against the reference ---------------------------------------------------------------------------------------------------

def _ref_remove(ref, which):
    ref._vectors = np.delete(ref._vectors, which, axis=0)


@needs_reference
def test_call_sequences_against_the_reference_class(fake):
    v, q = make_corpus(N, D, 8100)
    qs = make_queries(6, D, 8101)
    extra, _ = make_corpus(40, D, 8102)
    ours, ref = new_vb(v), ref_loader.make_reference_vectorbase(v.copy())

    def check():
        assert len(ours) == len(ref)
        for e in qs:
            same(ours.fuzzy_lookup_embedding(e, 9, 0.0), ref.fuzzy_lookup_embedding(e, 9, 0.0))
        sub = list(range(0, len(ref), 3))
        same(ours.fuzzy_lookup_embedding_in_subset(qs[0], sub, 5, 0.0), ref.fuzzy_lookup_embedding_in_subset(qs[0], sub, 5, 0.0))
        np.testing.assert_array_equal(np.asarray(ours.serialize()), ref.serialize())

    check()
    eng = ours._engine
    steps = [
        [0],
        [5, 5, -1, 17],  # duplicates, a negative ordinal
        np.arange(len(v)) % 4 == 1,  # (resized below)
        np.array([3, 2, 1], dtype=np.int32),
        7,  # a scalar, as np.delete takes it
        [],
    ]
    for which in steps:
        if isinstance(which, np.ndarray) and which.dtype == np.bool_:
            which = np.arange(len(ours)) % 4 == 1
        uploads = len(eng.uploads)
        n_before = len(ours)
        removed = ours.remove_rows(which)
        _ref_remove(ref, which)
        assert removed == n_before - len(ref)
        check()
        assert len(eng.uploads) == uploads, "a removal uploaded rows again"
    assert eng.compactions == 5
    # the ordinal shift: the row that was at 20 is now found at its new place
    probe = np.asarray(ours.serialize())[20].copy()
    ours.remove_rows([3, 4])
    assert ours.fuzzy_lookup_embedding(probe, 1, 0.0)[0].item == 18
    _ref_remove(ref, [3, 4])
    # append after a removal: only the new rows travel
    uploads = len(eng.uploads)
    ours.add_embeddings(None, extra)
    ref.add_embeddings(None, extra)
    check()
    assert eng.uploads[uploads:] == [(len(ref) - 40, 40)]
    ours.remove_at(len(ours) - 1)
    _ref_remove(ref, len(ref) - 1)
    check()
    # everything
    assert ours.remove_rows(np.ones(len(ours), dtype=bool)) == len(ref)
    _ref_remove(ref, np.ones(len(ref), dtype=bool))
    assert len(ours) == len(ref) == 0 and ours.fuzzy_lookup_embedding(qs[0], 3, 0.0) == []
    ours.add_embeddings(None, extra)
    ref.add_embeddings(None, extra)
    check()


@needs_reference
def test_np_delete_errors_are_the_reference_s(fake):
    v, q = make_corpus(50, D, 8200)
    ours, ref = new_vb(v), ref_loader.make_reference_vectorbase(v.copy())
    ours.fuzzy_lookup_embedding(q, 1, 0.0)
    for bad in ([50], [-51], [0, 99], np.array([1, 50]), [1.5], np.zeros(49, dtype=bool), np.zeros((50, 1), dtype=bool)):
        with pytest.raises((IndexError, ValueError)) as theirs:
            _ref_remove(ref, bad)
        with pytest.raises(type(theirs.value)):
            ours.remove_rows(bad)
        assert len(ours) == 50
    with pytest.raises(IndexError, match="Index 50 out of bounds for embedding index of size 50"):
        ours.remove_at(50)
    with pytest.raises(IndexError, match="Index -1 out of bounds"):
        ours.remove_at(-1)
    assert ours.remove_rows([]) == 0 and ours.remove_rows(np.zeros(50, dtype=bool)) == 0
    assert not hasattr(ours._engine, "compactions")


def test_an_index_that_never_reached_the_device_removes_on_the_host(fake):
    v, q = make_corpus(60, D, 8300)
    vb = new_vb(v)
    assert vb._engine is None and vb.remove_rows([0, 59]) == 2 and vb._engine is None
    np.testing.assert_array_equal(np.asarray(vb.serialize()), v[1:59])
    assert [r.item for r in vb.fuzzy_lookup_embedding(v[10], 1, 0.0)] == [9]
    assert vb._engine.uploads == [(0, 58)]


def test_the_row_message_map_and_the_caches_follow(fake):
    v, q = make_corpus(N, D, 8400)
    row_to_msg = (np.arange(N) // 3).astype(np.int64)
    row_to_msg[[7, 100]] = -1
    flags = np.arange(N) % 5 == 2
    vb = new_vb(v)
    vb.set_row_messages(row_to_msg)
    vb.lookup_messages_by_embedding(q, 10, 0.0)
    sub = list(range(0, N, 2))
    vb.fuzzy_lookup_embedding_in_subset(q, sub, 5, 0.0)
    vb.fuzzy_lookup_embedding_in_subset(q, sub, 5, 0.0)
    assert vb._subset_cache is not None and vb._row_messages_rows == N
    epoch = vb._removal_epoch
    assert vb.remove_rows(flags) == 60
    assert vb._subset_cache is None and vb._row_messages_rows == -1 and vb._removal_epoch == epoch + 1
    np.testing.assert_array_equal(vb._row_messages, np.delete(row_to_msg, np.flatnonzero(flags)))
    fresh = new_vb(np.delete(v, np.flatnonzero(flags), axis=0))
    fresh.set_row_messages(np.delete(row_to_msg, np.flatnonzero(flags)))
    assert pairs(vb.lookup_messages_by_embedding(q, 10, 0.0)) == pairs(fresh.lookup_messages_by_embedding(q, 10, 0.0))
    assert vb._row_messages_rows == len(vb) == N - 60
    short = list(range(0, N - 60, 2))
    assert pairs(vb.fuzzy_lookup_embedding_in_subset(q, short, 5, 0.0)) == pairs(fresh.fuzzy_lookup_embedding_in_subset(q, short, 5, 0.0))
    assert vb.remove_rows([]) == 0 and vb._removal_epoch == epoch + 1  # a no-op is no removal


def test_row_masks_made_before_a_removal_are_refused(fake):
    v, q = make_corpus(N, D, 8500)
    vb = new_vb(v)
    even = vb.row_mask(np.arange(N) % 2 == 0)
    few = vb.row_mask(np.arange(N) < 10)
    assert even.epoch == few.epoch == 0
    assert vb.remove_rows(few) == 10  # a RowMask of this index names the rows to remove
    np.testing.assert_array_equal(np.asarray(vb.serialize()), v[10:])
    for stale in (even, few):
        with pytest.raises(ValueError):
            vb.fuzzy_lookup_embedding_masked(q, stale, 3, 0.0)
    vb.add_embeddings(None, v[:10])
    assert len(vb) == N  # the old length again: still refused
    with pytest.raises(ValueError, match="removed"):
        vb.fuzzy_lookup_embedding_masked(q, even, 3, 0.0)
    with pytest.raises(ValueError, match="removed"):
        vb.remove_rows(even)
    with pytest.raises(ValueError, match="removed"):
        even & vb.row_mask(np.ones(N, dtype=bool))
    again = vb.row_mask(np.arange(N) % 2 == 0)
    assert again.epoch == 1 and len(vb.fuzzy_lookup_embedding_masked(q, again, 3, 0.0)) == 3
    other = new_vb(v)
    with pytest.raises(ValueError, match="another index"):
        vb.remove_rows(other.row_mask(np.ones(N, dtype=bool)))


def test_a_matrix_somebody_else_holds_is_not_edited(fake):
    v, q = make_corpus(80, D, 8600)
    flags = np.arange(80) % 3 == 0
    want = np.delete(v, np.flatnonzero(flags), axis=0)
    # the caller's own matrix, adopted by deserialize()
    data = v.copy()
    vb = new_vb()
    vb.deserialize(data)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    uploads = len(vb._engine.uploads)
    assert vb.remove_rows(flags) == 27
    np.testing.assert_array_equal(data, v)
    assert not np.shares_memory(vb._host, data) and not vb._handed_out
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    same(vb.fuzzy_lookup_embedding(q, 5, 0.0), new_vb(want).fuzzy_lookup_embedding(q, 5, 0.0))
    assert len(vb._engine.uploads) == uploads
    # a view of the index' own matrix, handed out by serialize()
    vb = new_vb(v)
    held = vb.serialize()
    snapshot = np.array(held)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    vb.remove_rows(flags)
    np.testing.assert_array_equal(np.asarray(held), snapshot)
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    # nobody holds it: compacted where it is
    vb = new_vb(v)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    buffer = vb._host
    vb.remove_rows(flags)
    assert vb._host is buffer
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    # rows edited through a view before the removal reach the mirror first
    vb = new_vb(v)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    m = vb.serialize()
    m[5] = v[6]
    vb.remove_rows([0])
    edited = v.copy()
    edited[5] = v[6]
    same(vb.fuzzy_lookup_embedding(q, 5, 0.0), new_vb(edited[1:]).fuzzy_lookup_embedding(q, 5, 0.0))


def test_a_device_only_corpus_stays_on_the_device(fake):
    v, q = make_corpus(90, D, 8700)
    vb = new_vb(keep_host_copy=False)
    vb.add_embeddings(None, v)
    assert vb._device_only is not None
    assert vb.remove_rows([1, 2, 89]) == 3
    assert vb._device_only is vb._engine.corpus and vb._host.shape[0] == 0 and len(vb) == 87 == vb._engine.rows
    assert vb._engine.mask_uploads == 1
    same(vb.fuzzy_lookup_embedding(q, 5, 0.0), new_vb(np.delete(v, [1, 2, 89], axis=0)).fuzzy_lookup_embedding(q, 5, 0.0))
    assert vb._device_only is not None


def test_a_device_group_removes_on_the_host_and_uploads_again(fake):
    v, q = make_corpus(120, D, 8800)
    vb = new_vb(v, devices=[0, 1])
    before = pairs(vb.fuzzy_lookup_embedding(q, 5, 0.0))
    assert before and not hasattr(vb._engine, "compact_rows")
    assert vb.remove_rows(np.arange(120) % 2 == 0) == 60
    want = v[1::2]
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    same(vb.fuzzy_lookup_embedding(q, 5, 0.0), new_vb(want).fuzzy_lookup_embedding(q, 5, 0.0))
    assert sum(e.rows for e in vb._engine.engines) == 60


# ---- the adapters ----------------------------------------------------------------------------------------------------------------------

RELATED_TERMS_DDL = "CREATE TABLE RelatedTermsFuzzy (term TEXT NOT NULL PRIMARY KEY, term_embedding BLOB NOT NULL)"  # schema.py:131-136
TERMS = ["apple pie", "banana bread", "cherry tart", "apple tart", "banana split", "date square", "elderflower cordial"]


@pytest.mark.skipif(not (ref_loader.reference_available() and ref_wrappers.consumers_available()), reason="the verbatim reference is only present in the build container")
def test_remove_term_over_the_reference_s_own_consumers(fake):
    import typeagent_py_amd.vectorbase as ours

    run = asyncio.run
    kept = ref_wrappers.load_consumers(ours, keep=True)
    settings = lambda: kept.fuzzyindex.TextEmbeddingIndexSettings(embedding_model=create_test_embedding_model(12), min_score=0.0, max_matches=7)
    try:
        db = sqlite3.connect(":memory:")
        db.execute(RELATED_TERMS_DDL)
        sql = kept.sqlite_reltermsindex.SqliteRelatedTermsFuzzy(db, settings())
        mem = kept.memory_reltermsindex.TermEmbeddingIndex(settings())
        with pytest.raises(NotImplementedError):
            run(sql.remove_term("apple pie"))
        assert not hasattr(mem, "remove_term")
        report = adapters.install_remove_term()
        assert report == {"patched": ["typeagent.storage.memory.reltermsindex.TermEmbeddingIndex", "typeagent.storage.sqlite.reltermsindex.SqliteRelatedTermsFuzzy"],
                          "skipped": {}}
        for idx in (sql, mem):
            run(idx.add_terms(TERMS))
            left = list(TERMS)
            for gone in ("cherry tart", "apple pie", "no such term", "elderflower cordial"):
                run(idx.remove_term(gone))
                if gone in left:
                    left.remove(gone)
                assert run(idx.size()) == len(left)
                if idx is sql:
                    twin_db = sqlite3.connect(":memory:")
                    twin_db.execute(RELATED_TERMS_DDL)
                    twin = type(idx)(twin_db, settings())
                else:
                    twin = type(idx)(settings())
                run(twin.add_terms(left))
                for probe in ("apple crumble", "cherry cake", gone):
                    got = run(idx.lookup_term(probe, 7, 0.0))
                    assert gone not in [t.text for t in got] or gone == "no such term"
                    assert [(t.text, t.weight) for t in got] == [(t.text, t.weight) for t in run(twin.lookup_term(probe, 7, 0.0))]
            assert len(idx._vector_base if idx is sql else idx._vectorbase) == len(left) == 4
        assert sql._terms_list == left and "apple pie" not in sql._added_terms
        assert sorted(r[0] for r in db.execute("SELECT term FROM RelatedTermsFuzzy")) == sorted(left)
        run(sql.add_terms(["apple pie"]))  # a removed term can come back
        assert run(sql.size()) == 5 and [t.text for t in run(sql.lookup_term("apple pie", 1, 0.0))] == ["apple pie"]
        adapters.uninstall_remove_term()
        with pytest.raises(NotImplementedError):
            run(sql.remove_term("apple tart"))
        assert not hasattr(mem, "remove_term")
    finally:
        adapters.uninstall_remove_term()
        kept.cleanup()


def test_install_remove_term_reports_what_it_cannot_import(monkeypatch):
    import sys

    for name in [m for m in sys.modules if m == "typeagent" or m.startswith("typeagent.")]:
        monkeypatch.delitem(sys.modules, name)
    monkeypatch.setitem(sys.modules, "typeagent", None)  # importing it raises ImportError
    report = adapters.install_remove_term()
    assert report["patched"] == [] and set(report["skipped"]) == {"typeagent.storage.memory.reltermsindex", "typeagent.storage.sqlite.reltermsindex"}
    adapters.uninstall_remove_term()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

def test_the_new_symbol_is_declared_bound_and_exported():
    import ctypes

    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert re.search(r"^int tavb_compact_rows\(tavb_ctx\* ctx, const uint32_t\* dev_remove_bits, int64_t rows,\s*void\* dev_dst[^;]*int64_t\* out_rows\);", header, re.M)
    assert "tavb_compact_rows" in _native.ABI_SYMBOLS
    lib = ctypes.CDLL(_native.library_path())
    assert hasattr(lib, "tavb_compact_rows")
    assert _native.load_library().tavb_version() == _native.ABI_VERSION == 7
    assert int(re.search(r"#define TAVB_KERNEL_COUNT (\d+)", header).group(1)) == 10
    # no context: refused with a message, nothing aborts
    kept = ctypes.c_int64(5)
    assert _native.load_library().tavb_compact_rows(None, None, 0, None, ctypes.byref(kept)) == -1
    assert b"null context" in _native.load_library().tavb_last_error()
