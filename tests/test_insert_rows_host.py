"""CPU suite: inserting and overwriting rows without a GPU.  The case table of tests/insert_rows_cases.py; `VectorBase.insert_rows` /
`insert_at` / `set_rows` on the suite's engine double -- which has neither `expand_rows` nor `scatter_rows`, so the class takes its host
route -- against numpy's own `np.insert` and index assignment; the bookkeeping around them (the row -> message map, the epoch of
`RowMask`, the subset cache, matrices somebody else holds, what travels to the device afterwards); and the C ABI's two additive symbols."""

import os
import re

import numpy as np
import pytest

from tests import insert_rows_cases as ic
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 300, 24


@pytest.fixture
def fake(monkeypatch):
    from typeagent_py_amd import multidevice

    monkeypatch.setattr(_native, "Engine", FakeEngine)
    monkeypatch.setattr(multidevice._native, "Engine", FakeEngine)


def new_vb(v=None, **kw) -> VectorBase:
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), **kw)
    if v is not None:
        vb.add_embeddings(None, np.array(v, dtype=np.float32))
    return vb


def pairs(res):
    return [(r.item, r.score) for r in res]


def same_lookups(vb, matrix, qs, row_to_msg=None):
    """Every lookup family of `vb` equals that of a fresh index over `matrix`."""
    fresh = new_vb(matrix)
    assert len(vb) == len(matrix)
    np.testing.assert_array_equal(np.asarray(vb.serialize()), matrix)
    for q in qs[:3]:
        assert pairs(vb.fuzzy_lookup_embedding(q, 9, 0.0)) == pairs(fresh.fuzzy_lookup_embedding(q, 9, 0.0))
    assert [pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, 7, 0.0)] == [pairs(r) for r in fresh.fuzzy_lookup_embeddings(qs, 7, 0.0)]
    sub = list(range(0, len(matrix), 3))
    assert pairs(vb.fuzzy_lookup_embedding_in_subset(qs[0], sub, 5, 0.0)) == pairs(fresh.fuzzy_lookup_embedding_in_subset(qs[0], sub, 5, 0.0))
    flags = np.arange(len(matrix)) % 2 == 0
    assert pairs(vb.fuzzy_lookup_embedding_masked(qs[1], vb.row_mask(flags), 5, 0.0)) == pairs(fresh.fuzzy_lookup_embedding_masked(qs[1], fresh.row_mask(flags), 5, 0.0))
    if row_to_msg is not None:
        fresh.set_row_messages(row_to_msg)
        assert pairs(vb.lookup_messages_by_embedding(qs[2], 10, 0.0)) == pairs(fresh.lookup_messages_by_embedding(qs[2], 10, 0.0))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_what_it_claims():
    cases = ic.cases()
    assert ic.CHUNK == _native.MASK_ROWS_PER_WORKGROUP and ic.CHUNK % ic.ODD_PASS != 0 and ic.ODD_PASS % ic.TILE == 0
    assert 150 <= len(cases) <= 250 and len({c.id for c in cases}) == len(cases)
    assert {c.rows for c in cases} == set(ic.ROWS) == {1, 2, 31, 32, 33, 64, 65, 16383, 16384, 16385, 2 * 16384 + 17}
    assert {(c.dim, c.dtype) for c in cases} == set(ic.SMALL_SHAPES + ic.WIDE_SHAPES + ic.NARROW_SHAPES)
    assert {c.rows for c in cases if c.dim == 1536} <= set(ic.AROUND_CHUNK) and {c.rows for c in cases if c.dim == 384} == set(ic.AROUND_CHUNK)
    assert {c.kind for c in cases} == set(ic.KINDS) and {c.route for c in cases} == set(ic.ROUTES)
    assert {c.pass_rows for c in cases if c.route == "in_place"} == set(ic.PASSES) | {4096}
    assert all(c.pass_rows == 0 for c in cases if c.route != "in_place")
    assert max((c.rows, c.dim) for c in cases) == (2 * ic.CHUNK + 17, 100)  # the longest corpus
    for rows in ic.ROWS:  # every kind that exists at a size is in the table at that size
        for kind in ic.KINDS:
            if kind != "block_longer_than_pass" and ic.insertion(kind, rows, 64) is not None:
                assert any(c.rows == rows and c.kind == kind for c in cases), (rows, kind)
    for route in ic.ROUTES:
        assert {c.kind for c in cases if c.route == route} >= set(ic.KINDS) - {"block_longer_than_pass"}
    many = [c for c in cases if c.route == "in_place" and c.rows > 4 * ic.effective_pass(c.pass_rows, c.dim, c.dtype)]
    assert len(many) >= 10  # many passes
    for c in cases:
        a, f = ic.at(c), ic.holes(c)
        m, n = len(a), c.rows - len(a)
        old, new = ic.old_matrix(c), ic.new_matrix(c)
        assert old.shape == (n, c.dim) and new.shape == (m, c.dim) and f.sum() == m
        for x in (old, new):
            assert np.array_equal(x.astype(np.float16).astype(np.float32), x)
        # the positions rebuilt by the documented rule are np.insert's
        pos = ic.positions_of(a, n)
        marks = np.insert(np.full(n, -1, dtype=np.int64), a, np.arange(m, dtype=np.int64)) if m else np.full(n, -1, dtype=np.int64)
        assert np.array_equal(np.flatnonzero(marks >= 0), np.sort(pos)) and np.array_equal(marks[pos], np.arange(m))
        np.testing.assert_array_equal(VectorBase._insert_positions(a, n, m) if m != 1 else pos, pos)
        p = ic.effective_pass(c.pass_rows, c.dim, c.dtype)
        assert p % ic.TILE == 0 and p >= ic.TILE
        if c.kind == "none":
            assert m == 0
        elif c.kind == "all":
            assert n == 0  # into an empty index
        elif c.kind == "all_but_first":
            assert n == 1 and not f[0]
        elif c.kind == "all_but_last":
            assert n == 1 and not f[-1]
        elif c.kind == "block_longer_than_pass":
            i = np.flatnonzero(f)
            assert i[-1] - i[0] + 1 == len(i) > p and c.route == "in_place" and 0 < i[0] and i[-1] < c.rows - 1
        elif c.kind == "block_over_chunk_edge":
            i = np.flatnonzero(f)
            assert i[0] < ic.CHUNK <= i[-1]
        elif c.kind == "repeated_at":
            assert m > 1 and len(set(a.tolist())) == 1
        elif c.kind == "unsorted_at":
            assert (np.diff(pos) < 0).any() and len(set((a % max(n, 1)).tolist())) < m
    assert any((ic.at(c) < 0).any() for c in cases if c.kind == "unsorted_at")
    for dim in (8, 100, 384, 1536, 33):
        both = np.concatenate([ic.base_matrix(dim), -ic.base_matrix(dim) - np.eye(1, dim, 1, dtype=np.float32)])
        assert len(np.unique(both[:, :3], axis=0)) == len(both)  # no two rows alike, old or new: a misplaced row shows


def test_the_twin_of_the_passes_equals_np_insert():
    """The in-place algorithm as the library runs it -- passes of whole tiles, FROM THE TAIL, down to the tile of the first hole; a pass'
    old rows staged, then written to the rows of the pass that are no hole -- restated in numpy over the table, with the two facts the
    safety argument rests on."""
    for c in ic.cases():
        if c.route != "in_place" or c.dim > 100:
            continue
        f = ic.holes(c)
        n = c.rows - int(f.sum())
        a = np.full(c.rows, -7, dtype=np.int64)
        a[:n] = np.arange(n)
        if f.any() and int(np.argmax(f)) < n:
            p = ic.effective_pass(c.pass_rows, c.dim, c.dtype)
            start = int(np.argmax(f)) // ic.TILE * ic.TILE
            for r0 in reversed(range(start, c.rows, p)):
                r1 = min(r0 + p, c.rows)
                o0, o1 = int((~f[:r0]).sum()), int((~f[:r1]).sum())
                assert o0 <= r0 and o1 <= r1  # rows only move up: later passes read only below o0 <= r0, and nothing below r0 is written yet
                staged = a[o0:o1].copy()
                a[r0:r1][~f[r0:r1]] = staged
        np.testing.assert_array_equal(a[~f], np.arange(n), err_msg=c.id)


# ---- the class against numpy -------------------------------------------------------------------------------------------------------------

def test_call_sequences_against_np_insert(fake):
    v, _ = make_corpus(N, D, 9100)
    qs = make_queries(6, D, 9101)
    extra, _ = make_corpus(64, D, 9102)
    vb, model = new_vb(v), v.copy()
    same_lookups(vb, model, qs)
    eng = vb._engine
    steps = [
        (0, extra[:1]),
        (len(v) + 1, extra[1:4]),  # at == len(self): an append
        (-1, extra[4]),  # a negative position, one row as [dim]
        ([5, 5, 2, -3], extra[5:9]),  # equal positions keep their order; unsorted; negative
        (np.array([7], dtype=np.int32), extra[9:12]),  # one position in a sequence: all rows in front of it
        ([10, 200, 30], extra[12]),  # one row, many positions
        ([], extra[:0]),
    ]
    for at, rows in steps:
        before, uploads = len(vb), len(eng.uploads)
        want = np.insert(model, at, rows, axis=0)
        assert vb.insert_rows(at, rows) == len(want) - before
        model = want
        same_lookups(vb, model, qs)
        if len(want) > before:  # the host route: the upload starts at the first new row, never at row 0 unless that is new
            first = int(np.argmax((np.insert(np.zeros(before), at, 1) > 0)))
            assert eng.uploads[uploads:] == [(first, len(want) - first)]
    # the ordinal shift: the row that was at 20 is found two places up
    probe = model[20].copy()
    vb.insert_rows([3, 4], extra[20:22])
    assert vb.fuzzy_lookup_embedding(probe, 1, 0.0)[0].item == 22
    model = np.insert(model, [3, 4], extra[20:22], axis=0)
    # insert_at: the reference's commented method
    vb.insert_at(0, extra[30])
    vb.insert_at(len(vb), [extra[31], extra[32]])
    vb.insert_at(17, [extra[33]])
    model = np.vstack([extra[30:31], model, extra[31:33]])
    model = np.vstack([model[:17], extra[33:34], model[17:]])
    same_lookups(vb, model, qs)
    # overwrite
    for which, rows in (([3], extra[40:41]), ([-1, 0, 5], extra[41:44]), (np.arange(len(model)) % 50 == 7, extra[50]), ([8, 9, 8], extra[44:47])):
        count = len(vb)
        written = vb.set_rows(which, rows)
        model[which] = rows
        assert len(vb) == count and written == len(set(np.arange(count)[which].tolist()))
        same_lookups(vb, model, qs)
    np.testing.assert_array_equal(model[8], extra[46])  # duplicates: the last one wins (numpy's rule too)


def test_insert_into_an_empty_index_learns_the_width(fake):
    v, q = make_corpus(20, D, 9200)
    vb = new_vb()
    assert vb._embedding_size == 0 and vb.insert_rows(0, v[:3]) == 3 and vb._embedding_size == D
    assert vb.insert_rows([0, 0, 3], v[3:6]) == 3
    np.testing.assert_array_equal(np.asarray(vb.serialize()), np.insert(v[:3], [0, 0, 3], v[3:6], axis=0))
    vb2 = new_vb()
    vb2.insert_rows([0, 0, 0], v[:3], row_messages=[4, 5, 6])
    np.testing.assert_array_equal(np.asarray(vb2.serialize()), v[:3])
    assert vb2._row_messages.tolist() == [4, 5, 6]
    vb3 = new_vb()
    with pytest.raises(IndexError):
        vb3.insert_rows(1, v[:1])


def test_numpy_s_errors(fake):
    v, q = make_corpus(50, D, 9300)
    vb, model = new_vb(v), v.copy()
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    row = v[:1]
    for bad_at, rows in ((51, row), (-51, row), ([0, 99], v[:2]), ([1.0, 2.0], v[:2])):
        with pytest.raises(IndexError):
            np.insert(model, bad_at, rows, axis=0)
        with pytest.raises(IndexError):
            vb.insert_rows(bad_at, rows)
    # where numpy is laxer or says it otherwise (a sequence is wrapped but not checked below -n; a float scalar is a TypeError): IndexError
    for bad_at, rows in ((np.array([1, -60]), v[:2]), (1.5, row), ([-51], row)):
        with pytest.raises(IndexError):
            vb.insert_rows(bad_at, rows)
    for at, rows in ((3, np.zeros((1, D + 1), dtype=np.float32)), ([1, 2, 3], v[:2]), (3, np.zeros((2, 2, D), dtype=np.float32))):
        with pytest.raises(ValueError):
            np.insert(model, at, rows, axis=0)
        with pytest.raises(ValueError):
            vb.insert_rows(at, rows)
    with pytest.raises(ValueError):
        vb.insert_rows([1, 2], v[:2], row_messages=[1, 2, 3])
    with pytest.raises(IndexError, match="Index 51 out of bounds for insertion in embedding index of size 50"):
        vb.insert_at(51, v[0])
    with pytest.raises(IndexError, match="Index -1 out of bounds for insertion"):
        vb.insert_at(-1, v[0])
    for bad in ([50], [-51], [0, 99], [1.5], np.zeros(49, dtype=bool)):
        with pytest.raises(IndexError):
            model[bad] = row
        with pytest.raises(IndexError):
            vb.set_rows(bad, row)
    for which, rows in (([1, 2, 3], v[:2]), ([1], np.zeros((1, D + 1), dtype=np.float32))):
        with pytest.raises(ValueError):
            model[which] = rows
        with pytest.raises(ValueError):
            vb.set_rows(which, rows)
    other = new_vb(v)
    with pytest.raises(ValueError, match="another index"):
        vb.set_rows(other.row_mask(np.ones(50, dtype=bool)), row)
    assert vb.set_rows([], v[:0]) == 0 and vb.set_rows(np.zeros(50, dtype=bool), row) == 0
    assert len(vb) == 50 and vb._removal_epoch == 0
    np.testing.assert_array_equal(np.asarray(vb.serialize()), v)
    np.testing.assert_array_equal(model, v)


def test_the_row_message_map_the_caches_and_the_masks_follow(fake):
    v, q = make_corpus(N, D, 9400)
    extra, _ = make_corpus(8, D, 9401)
    qs = make_queries(4, D, 9402)
    row_to_msg = (np.arange(N) // 3).astype(np.int64)
    row_to_msg[[7, 100]] = -1
    vb = new_vb(v)
    vb.set_row_messages(row_to_msg)
    vb.lookup_messages_by_embedding(q, 10, 0.0)
    sub = list(range(0, N, 2))
    vb.fuzzy_lookup_embedding_in_subset(q, sub, 5, 0.0)
    vb.fuzzy_lookup_embedding_in_subset(q, sub, 5, 0.0)
    even = vb.row_mask(np.arange(N) % 2 == 0)
    assert vb._subset_cache is not None and vb._row_messages_rows == N
    # overwrite: nothing but the rows changes
    assert vb.set_rows(even, v[1::2]) == N // 2
    model = v.copy()
    model[0::2] = v[1::2]  # a RowMask's rows in ascending order take the rows in order
    assert vb._subset_cache is not None and vb._row_messages_rows == N and vb._removal_epoch == 0
    assert pairs(vb.fuzzy_lookup_embedding_masked(q, even, 3, 0.0)) == pairs(new_vb(model).fuzzy_lookup_embedding_masked(q, np.arange(N) % 2 == 0, 3, 0.0))
    same_lookups(vb, model, qs, row_to_msg)
    # insert: messages given, and the default
    at = [0, 150, 150, N]
    assert vb.insert_rows(at, extra[:4], row_messages=[90, 91, 92, 93]) == 4
    assert vb._subset_cache is None and vb._row_messages_rows == -1 and vb._removal_epoch == 1
    row_to_msg = np.insert(row_to_msg, at, [90, 91, 92, 93])
    model = np.insert(model, at, extra[:4], axis=0)
    np.testing.assert_array_equal(vb._row_messages, row_to_msg)
    same_lookups(vb, model, qs, row_to_msg)
    assert vb.insert_rows(5, extra[4:6]) == 2 and vb.insert_rows(9, extra[6], row_messages=44) == 1
    row_to_msg = np.insert(np.insert(row_to_msg, 5, [-1, -1]), 9, 44)
    model = np.insert(np.insert(model, 5, extra[4:6], axis=0), 9, extra[6], axis=0)
    np.testing.assert_array_equal(vb._row_messages, row_to_msg)
    same_lookups(vb, model, qs, row_to_msg)
    # the handle from before the insertions is refused, whatever the length; one made now is not
    with pytest.raises(ValueError):
        vb.fuzzy_lookup_embedding_masked(q, even, 3, 0.0)
    vb.remove_rows(np.arange(len(vb)) >= N)
    assert len(vb) == N
    with pytest.raises(ValueError, match="removed"):
        vb.fuzzy_lookup_embedding_masked(q, even, 3, 0.0)
    vb.remove_rows([0])
    vb.insert_rows(0, extra[:1])
    assert len(vb) == N
    with pytest.raises(ValueError, match="this RowMask was built before rows were inserted into the index: build it again"):
        vb.set_rows(even, v[1::2])
    epoch = vb._removal_epoch
    again = vb.row_mask(np.arange(N) % 2 == 0)
    assert vb.insert_rows([], extra[:0]) == 0 and vb._removal_epoch == epoch  # a no-op is no insertion
    assert len(vb.fuzzy_lookup_embedding_masked(q, again, 3, 0.0)) == 3
    # a map that did not exist: the old rows have no message
    vb2 = new_vb(v[:5])
    vb2.insert_rows(2, extra[:1], row_messages=[8])
    assert vb2._row_messages.tolist() == [-1, -1, 8, -1, -1, -1]


def test_a_matrix_somebody_else_holds_is_not_opened_up(fake):
    v, q = make_corpus(80, D, 9500)
    extra, _ = make_corpus(5, D, 9501)
    at = [0, 40, 40, 80, 17]
    want = np.insert(v, at, extra, axis=0)
    # the caller's own matrix, adopted by deserialize(): np.insert leaves it alone
    data = v.copy()
    vb = new_vb()
    vb.deserialize(data)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    assert vb.insert_rows(at, extra) == 5
    np.testing.assert_array_equal(data, v)
    assert not np.shares_memory(vb._host, data) and not vb._handed_out
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    assert pairs(vb.fuzzy_lookup_embedding(q, 5, 0.0)) == pairs(new_vb(want).fuzzy_lookup_embedding(q, 5, 0.0))
    # ... while index assignment writes it, as the reference's `_vectors[i] = row` does
    data = v.copy()
    vb = new_vb()
    vb.deserialize(data)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    uploads = len(vb._engine.uploads)
    vb.set_rows([3, 70], extra[:2])
    np.testing.assert_array_equal(data[[3, 70]], extra[:2])
    assert [r.item for r in vb.fuzzy_lookup_embedding(extra[1], 1, 0.0)] == [70]
    assert vb._engine.uploads[uploads:] == [(3, 77)]  # from the first written row on, once
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    assert len(vb._engine.uploads) == uploads + 1
    # a view of the index' own matrix, handed out by serialize()
    vb = new_vb(v)
    held = vb.serialize()
    snapshot = np.array(held)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    vb.insert_rows(at, extra)
    np.testing.assert_array_equal(np.asarray(held), snapshot)
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    # nobody holds it and there is room: opened up where it is
    vb = new_vb()
    vb.add_embeddings(None, v[:40])
    vb.add_embeddings(None, v[40:70])  # (the growth buffer now has spare rows)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    buffer = vb._host
    assert buffer.shape[0] >= 75
    vb.insert_rows([0, 40, 40, 70, 17], extra)
    assert vb._host is buffer
    np.testing.assert_array_equal(np.asarray(vb.serialize()), np.insert(v[:70], [0, 40, 40, 70, 17], extra, axis=0))
    # ... in blocks from the tail, whatever their size: blocks with holes, blocks without, blocks of one row
    for block_rows in (1, 3, 7, 16, 1000):
        for at2 in ([0], [69], [70], [0, 40, 40, 70, 17], [3, 3, 3, 3, 3], [66, 20, 21, 22, 1]):
            vb = new_vb()
            vb._host_block_bytes = block_rows * D * 4
            vb.add_embeddings(None, v[:40])
            vb.add_embeddings(None, v[40:70])
            buffer = vb._host
            vb.insert_rows(at2, extra[: len(at2)])
            assert vb._host is buffer
            np.testing.assert_array_equal(np.asarray(vb.serialize()), np.insert(v[:70], at2, extra[: len(at2)], axis=0))
    # rows edited through a view before the insertion are not lost
    vb = new_vb(v)
    vb.fuzzy_lookup_embedding(q, 1, 0.0)
    m = vb.serialize()
    m[5] = v[6]
    vb.insert_rows(0, extra[:1])
    edited = v.copy()
    edited[5] = v[6]
    assert pairs(vb.fuzzy_lookup_embedding(q, 5, 0.0)) == pairs(new_vb(np.insert(edited, 0, extra[:1], axis=0)).fuzzy_lookup_embedding(q, 5, 0.0))


def test_an_index_that_never_reached_the_device_edits_the_host(fake):
    v, q = make_corpus(60, D, 9600)
    vb = new_vb(v[:58])
    assert vb._engine is None and vb.insert_rows([0, 58], v[58:]) == 2 and vb.set_rows([1], v[:1]) == 1 and vb._engine is None
    want = np.insert(v[:58], [0, 58], v[58:], axis=0)
    want[1] = v[0]
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    assert [r.item for r in vb.fuzzy_lookup_embedding(v[10], 1, 0.0)] == [11]
    assert vb._engine.uploads == [(0, 60)]


def test_a_device_group_takes_the_host_route(fake):
    v, q = make_corpus(120, D, 9700)
    extra, _ = make_corpus(3, D, 9701)
    want = np.insert(v, [5, 5, 119], extra, axis=0)
    vb = new_vb(v, devices=[0, 1])
    assert vb.fuzzy_lookup_embedding(q, 5, 0.0) and not hasattr(vb._engine, "expand_rows")
    assert vb.insert_rows([5, 5, 119], extra) == 3 and vb.set_rows([0, -1], extra[:2]) == 2
    want[[0, -1]] = extra[:2]
    np.testing.assert_array_equal(np.asarray(vb.serialize()), want)
    assert pairs(vb.fuzzy_lookup_embedding(q, 5, 0.0)) == pairs(new_vb(want).fuzzy_lookup_embedding(q, 5, 0.0))
    assert sum(e.rows for e in vb._engine.engines) == 123


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------------

def test_the_new_symbols_are_declared_bound_and_exported():
    import ctypes

    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert re.search(r"^int tavb_expand_rows\(tavb_ctx\* ctx, const uint32_t\* dev_hole_bits, int64_t new_rows,\s*void\* dev_dst[^;]*int64_t\* out_old_rows\);", header, re.M)
    assert re.search(r"^int tavb_scatter_rows\(tavb_ctx\* ctx, const float\* rows_host_f32, int64_t n, int32_t dim,\s*const int32_t\* dev_positions_i32\);", header, re.M)
    lib = ctypes.CDLL(_native.library_path())
    for name in ("tavb_expand_rows", "tavb_scatter_rows"):
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    assert hasattr(_native.Engine, "expand_rows") and hasattr(_native.Engine, "scatter_rows")
    assert _native.load_library().tavb_version() == _native.ABI_VERSION == 7
    assert int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1)) == 7
    assert int(re.search(r"#define TAVB_KERNEL_COUNT (\d+)", header).group(1)) == 10
    # no context: refused with a message, nothing aborts
    old = ctypes.c_int64(5)
    assert _native.load_library().tavb_expand_rows(None, None, 0, None, ctypes.byref(old)) == -1
    assert b"null context" in _native.load_library().tavb_last_error()
    assert _native.load_library().tavb_scatter_rows(None, None, 0, 4, None) == -1
    assert b"null context" in _native.load_library().tavb_last_error()
