"""CPU suite: `RowMask` handles carried through row edits without a GPU -- `remove_rows(carry=)`, `insert_rows(carry=, carry_new=)` and
`extend_masks` on their host route (an index that never reached a device, handles that hold a host list only) against numpy's delete /
insert / concatenate over the case table of tests/mask_carry_cases.py; the table itself; the refusals, which come before anything is
edited; and the C ABI's additive symbol."""

import os
import re

import numpy as np
import pytest

from tests import mask_carry_cases as mc
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native
from typeagent_py_amd.vectorbase import RowMask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def new_vb(v=None) -> VectorBase:
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    if v is not None:
        vb.add_embeddings(None, np.array(v, dtype=np.float32))
    return vb


def host_handle(vb: VectorBase, bools: np.ndarray) -> RowMask:
    """A handle with a host list only: what `row_mask` makes where no engine expands masks."""
    flat = np.flatnonzero(bools)
    return RowMask(vb, len(bools), len(flat), flat=flat)


def bools_of(vb: VectorBase, h: RowMask) -> np.ndarray:
    assert h.rows == len(vb) and h.epoch == vb._removal_epoch and h.count == len(h.flat()) and h._plans == {}
    return vb._mask_bools(h)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_what_it_claims():
    cases = mc.cases()
    assert len({c.id for c in cases}) == len(cases)
    for mode, kinds in (("remove", mc.REMOVE_KINDS), ("insert", mc.INSERT_KINDS), ("append", mc.APPEND_KINDS)):
        mine = [c for c in cases if c.mode == mode]
        assert {c.rows for c in mine} == set(mc.ROWS) and {c.kind for c in mine} == set(kinds), mode
        assert {c.n_masks for c in mine} == set(mc.MASK_COUNTS) and {c.dtype for c in mine} == set(mc.DTYPES), mode
        exists = {"remove": lambda k, n: mc.removal(k, n) is not None, "insert": lambda k, n: mc.insertion(k, n) is not None,
                  "append": lambda k, n: mc.appended(k, n) is not None}[mode]
        for rows in mc.AROUND_CHUNK:  # every kind that exists there, at every chunk edge; all of them beyond the first chunk
            assert {c.kind for c in mine if c.rows == rows} == {k for k in kinds if exists(k, rows)}, (mode, rows)
        assert {c.kind for c in mine if c.rows == 2 * mc.CHUNK + 17} == set(kinds), mode
        if mode != "remove":
            for rows in mc.AROUND_CHUNK:
                for kind in (k for k in kinds if exists(k, rows)):
                    assert {c.fill for c in mine if c.rows == rows and c.kind == kind} == {False, True}, (mode, rows, kind)
    assert len(mc.REMOVE_KINDS) == 14 and mc.ROWS == (1, 2, 31, 32, 33, 63, 64, 65, 16383, 16384, 16385, 2 * 16384 + 17)
    # the carried masks: every kind among eight handles; the removal mask itself and its complement
    c = next(c for c in cases if c.mode == "remove" and c.kind == "random_50" and c.n_masks == 8 and c.rows > mc.CHUNK)
    ms, f = mc.masks(c), mc.flags(c)
    assert len(ms) == 8 and not ms[0].any() and ms[1].all() and np.array_equal(ms[2], f) and np.array_equal(ms[3], ~f)
    assert np.flatnonzero(ms[4]).tolist() == [c.rows - 1] and np.flatnonzero(ms[5]).tolist() == [0]
    assert 0 < ms[6].mean() < 0.03 and 0.4 < ms[7].mean() < 0.6
    seventeen = mc.masks(next(c for c in cases if c.n_masks == 17))
    assert len(seventeen) == 17 and not np.array_equal(seventeen[7], seventeen[15])  # (the random kinds differ from turn to turn)


def test_the_table_s_flags_and_numpy_agree():
    """`flags` is what the device is handed; `expected` is numpy's own delete / insert.  They describe the same edit: a removal keeps the
    clear flags' rows in order; an insertion leaves the old bits, in order, at the clear flags and the fill at the set ones."""
    for c in mc.cases():
        want = mc.expected(c)
        assert all(len(w) == mc.new_rows(c) for w in want), c.id
        if c.mode == "append":
            continue
        f = mc.flags(c)
        assert len(f) == (c.rows if c.mode == "remove" else mc.new_rows(c)) and int((~f).sum()) == (mc.new_rows(c) if c.mode == "remove" else c.rows), c.id
        for b, w in zip(mc.masks(c), want):
            if c.mode == "remove":
                assert np.array_equal(w, b[~f]), c.id
            else:
                assert np.array_equal(w[~f], b) and (w[f] == c.fill).all(), c.id
    # the kinds the issue names: equal positions among the scattered ones, a block over the chunk edge, an insertion that more than doubles
    at, m = mc.insertion("scattered", 65)
    assert len(at) == m and len(set(at.tolist())) < m
    assert np.flatnonzero(mc.flags(mc.Case("insert", mc.CHUNK, "block_over_chunk_edge", 1, False, "fp16"))).tolist() == list(range(mc.CHUNK - 50, mc.CHUNK + 50))
    assert mc.insertion("outgrow", 64)[1] > 64
    assert mc.appended("over_chunk_edge", mc.CHUNK - 1) == 4 and mc.appended("over_chunk_edge", mc.CHUNK + 1) == mc.CHUNK + 2


# ---- the host route, with no engine ---------------------------------------------------------------------------------------------------------

def _run_host(c: mc.Case):
    vb = new_vb(mc.old_matrix(c)[:, :8])
    handles = [host_handle(vb, b) for b in mc.masks(c)]
    epoch = vb._removal_epoch
    if c.mode == "remove":
        f = mc.flags(c)
        assert vb.remove_rows(f, carry=handles) == int(f.sum())
        changed = bool(f.any())
    elif c.mode == "insert":
        at, m = mc.insertion(c.kind, c.rows)
        assert vb.insert_rows(at, mc.new_vectors(c)[:, :8], carry=handles, carry_new=c.fill) == m
        changed = True
    else:
        vb.add_embeddings(None, np.array(mc.new_vectors(c)[:, :8]))
        assert vb.extend_masks(*handles, new=c.fill) is None
        changed = False
    assert vb._engine is None, "the host route of an index without an engine must not make one"
    assert len(vb) == mc.new_rows(c) and vb._removal_epoch == epoch + int(changed)
    for h, want in zip(handles, mc.expected(c)):
        assert np.array_equal(bools_of(vb, h), want), c.id
        assert h.dev_bits is None and h.dev_rows is None and h.span is None


@pytest.mark.parametrize("mode", ["remove", "insert", "append"])
def test_the_host_route_equals_numpy_at_every_case(mode):
    for c in mc.cases():
        if c.mode == mode:
            _run_host(c)


def test_a_handle_that_names_the_removed_rows_becomes_the_empty_mask():
    vb = new_vb(mc.base_matrix()[:100, :8])
    which = host_handle(vb, np.arange(100) % 3 == 0)
    other = host_handle(vb, np.arange(100) % 2 == 0)
    assert vb.remove_rows(which, carry=[which, other, which]) == 34  # (a handle named twice is carried once)
    assert which.count == 0 and which.rows == 66 and not bools_of(vb, which).any()
    assert np.array_equal(bools_of(vb, other), np.delete(np.arange(100) % 2 == 0, np.flatnonzero(np.arange(100) % 3 == 0)))
    # integer ordinals with np.delete's rules, one handle not in a list
    assert vb.remove_rows([0, -1, 0], carry=other) == 2
    assert np.array_equal(bools_of(vb, other), np.delete(np.arange(100) % 2 == 0, np.flatnonzero(np.arange(100) % 3 == 0))[1:-1])


def test_nothing_removed_or_inserted_changes_nothing():
    vb = new_vb(mc.base_matrix()[:40, :8])
    h = host_handle(vb, np.arange(40) < 7)
    flat = h.flat()
    assert vb.remove_rows([], carry=[h]) == 0 and vb.remove_rows(np.zeros(40, dtype=bool), carry=[h]) == 0
    assert vb.insert_rows(3, np.zeros((0, 8), dtype=np.float32), carry=[h]) == 0
    vb.extend_masks(h, new=True)  # already at the current length: left alone
    assert h.rows == 40 and h.epoch == 0 == vb._removal_epoch and h.flat() is flat


def test_an_empty_index_grows_under_a_carried_handle():
    vb = new_vb()
    vb._set_embedding_size(8)
    h = vb.row_mask(np.zeros(0, dtype=bool))
    assert vb.insert_rows(0, mc.base_matrix()[:3, :8], carry=[h], carry_new=True) == 3
    assert bools_of(vb, h).tolist() == [True] * 3
    vb.add_embeddings(None, np.array(mc.base_matrix()[:2, :8]))
    vb.extend_masks(h)
    assert bools_of(vb, h).tolist() == [True] * 3 + [False] * 2


# ---- refusals: before anything is edited ----------------------------------------------------------------------------------------------------

def test_refusals_come_before_the_edit():
    v = mc.base_matrix()[:50, :8]
    vb, other = new_vb(v), new_vb(v)
    good = host_handle(vb, np.arange(50) % 2 == 0)
    foreign = host_handle(other, np.ones(50, dtype=bool))
    short = host_handle(vb, np.ones(49, dtype=bool))
    rows = np.array(v[:2])

    def untouched():
        assert len(vb) == 50 and vb._removal_epoch == 0 and good.rows == 50 and good.epoch == 0 and good.count == 25
        np.testing.assert_array_equal(np.asarray(vb.serialize()), v)

    for bad, match in ((foreign, "another index"), (short, "covers 49 rows")):
        with pytest.raises(ValueError, match=match):
            vb.remove_rows([1, 2], carry=[good, bad])
        with pytest.raises(ValueError, match=match):
            vb.insert_rows(5, rows, carry=[good, bad])
        untouched()
    with pytest.raises(TypeError, match="RowMask"):
        vb.remove_rows([1], carry=[np.ones(50, dtype=bool)])
    with pytest.raises(TypeError, match="RowMask"):
        vb.extend_masks(np.ones(50, dtype=bool))
    with pytest.raises(ValueError, match="another index"):
        vb.extend_masks(good, foreign)
    untouched()
    # a stale epoch: an edit that was not handed the handle (the length is the old one again, as in the removal tests)
    stale = host_handle(vb, np.arange(50) < 5)
    assert vb.remove_rows([0], carry=[good]) == 1
    vb.add_embeddings(None, rows[:1])
    vb.extend_masks(good)
    assert len(vb) == 50 and good.rows == 50 and good.epoch == 1 and good.count == 24
    for call in (lambda: vb.remove_rows([3], carry=[good, stale]), lambda: vb.insert_rows(0, rows, carry=[stale]), lambda: vb.extend_masks(good, stale)):
        with pytest.raises(ValueError, match="removed from"):
            call()
    assert len(vb) == 50 and vb._removal_epoch == 1 and good.rows == 50 and good.epoch == 1
    # extend_masks takes only handles no longer than the index
    long_one = host_handle(vb, np.ones(51, dtype=bool))
    vb.add_embeddings(None, rows[:1])
    vb.extend_masks(long_one)  # (51 rows by now: left alone)
    assert long_one.rows == 51 and long_one.count == 51
    longer = host_handle(vb, np.ones(len(vb) + 1, dtype=bool))
    with pytest.raises(ValueError, match=f"covers {len(vb) + 1} rows"):
        vb.extend_masks(long_one, longer)


def test_without_carry_today_s_refusals_stay():
    v = mc.base_matrix()[:30, :8]
    vb = new_vb(v)
    a, b = host_handle(vb, np.arange(30) % 2 == 0), host_handle(vb, np.arange(30) % 3 == 0)
    assert vb.remove_rows([4]) == 1
    assert vb.remove_rows([4], carry=()) == 1
    vb.add_embeddings(None, np.array(v[:2]))
    for h in (a, b):
        with pytest.raises(ValueError, match="removed from"):
            vb._resolve_mask(h)
    assert vb.remove_rows([28, 29]) == 2
    c = host_handle(vb, np.ones(28, dtype=bool))
    assert vb.insert_rows(0, np.array(v[:1])) == 1
    with pytest.raises(ValueError):
        vb._resolve_mask(c)
    d = host_handle(vb, np.ones(29, dtype=bool))
    vb.add_embeddings(None, np.array(v[:1]))
    with pytest.raises(ValueError, match="covers 29 rows"):
        vb._resolve_mask(d)  # an append alone: refused until extend_masks
    vb.extend_masks(d)
    assert vb._resolve_mask(d) is d and d.rows == 30 and d.count == 29
    # set_rows bumps nothing and takes no carry
    assert vb.set_rows([0], np.array(v[3:4])) == 1 and vb._resolve_mask(d) is d
    with pytest.raises(TypeError):
        vb.set_rows([0], np.array(v[3:4]), carry=[d])


def test_more_than_eight_handles_are_folded_in_groups_on_the_device_route():
    """`_remap_on_device` with an engine double: 17 handles go as 8 + 8 + 1, every call with the same flags and sizes and its handles' counts."""
    calls = []

    class Eng:
        def mask_remap(self, mode, dev_flags, old, new, bits, fill, counts=None):
            calls.append((mode, dev_flags, old, new, list(bits), fill, list(counts)))
            return [(f"rows{b}", 0, f"bits{b}", None) for b in bits]

    vb = new_vb(mc.base_matrix()[:10, :8])
    handles = [host_handle(vb, np.arange(10) < i % 10) for i in range(17)]
    for i, h in enumerate(handles):
        h.dev_bits = i
    out = vb._remap_on_device(Eng(), _native.REMAP_REMOVE, "flags", 10, 7, handles, False)
    assert [len(c[4]) for c in calls] == [8, 8, 1] and all(c[:4] == (0, "flags", 10, 7) and c[5] is False for c in calls)
    assert [b for c in calls for b in c[4]] == list(range(17)) and [n for c in calls for n in c[6]] == [h.count for h in handles]
    assert [o[2] for o in out] == [f"bits{i}" for i in range(17)]


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------

def lib_version() -> int:
    return _native.load_library().tavb_version()


def test_the_new_symbol_is_declared_bound_and_exported():
    """The symbol is additive, as the edits' own symbols were: a library of the same ABI version gains an entry point, nothing else moves."""
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert "tavb_mask_remap" in _native.ABI_SYMBOLS and re.search(r"\bint tavb_mask_remap\(tavb_ctx\* ctx, int32_t mode,", header)
    assert _native.ABI_VERSION == lib_version() == 7 and (_native.REMAP_REMOVE, _native.REMAP_INSERT, _native.REMAP_APPEND) == (0, 1, 2)
    for name, value in (("REMOVE", 0), ("INSERT", 1), ("APPEND", 2)):
        assert re.search(rf"#define TAVB_REMAP_{name} {value}\b", header)
    lib = _native.load_library()
    infos = (_native.MaskInfo * 1)()
    ptrs = (_native.c_void_p * 1)(None)
    assert lib.tavb_mask_remap(None, 0, None, 0, 0, ptrs, ptrs, 1, 0, None, None, infos) == -1 and b"null context" in lib.tavb_last_error()
