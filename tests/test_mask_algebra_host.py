"""CPU suite: the scope algebra without a GPU -- the case table of tests/mask_algebra_cases.py pinned against brute-force numpy (the twins
of `mask_combine_kernel` and `mask_from_ranges_kernel`, whole words, tail bits zero), `RowMask`'s operators, `VectorBase.intersect_masks`
/ `union_masks` / `range_mask` and `adapters.scope_collections` / `lookup_messages_in_scope` on the engine double and on a device group
of doubles against the bool-array compositions they are defined as, their argument errors, `scope_collections` against the reference's
own `TextRangesInScope.is_range_in_scope`, and the C ABI's two additive symbols."""

import os
import re
import types
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import ref_loader
from tests import mask_algebra_cases as mc
from tests import message_scope_cases as sc
from tests.test_message_scope_host import BUILDERS, pairs, single
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D = 240, 32
NEW_SYMBOLS = ("tavb_mask_from_ranges", "tavb_mask_combine")


# ---- the table itself ------------------------------------------------------------------------------------------------------------------

def test_the_table_covers_what_it_claims():
    assert mc.C == _native.MASK_ROWS_PER_WORKGROUP and mc.LDS_RANGES == _native.SCOPE_LDS_RANGES
    assert (mc.AND, mc.OR, mc.ANDNOT) == (_native.MASK_AND, _native.MASK_OR, _native.MASK_ANDNOT)
    assert mc.ROWS == (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, mc.C - 1, mc.C, mc.C + 1, 3 * mc.C + 17)
    assert max(mc.OPERAND_COUNTS) == _native.MAX_MASK_OPERANDS == 8 and _native.MAX_SCOPE_COLLECTIONS == 8
    for rows in mc.ROWS:
        ms = {k: mc.operand(k, rows, 1) for k in mc.KINDS}
        assert not ms["none"].any() and ms["all"].all() and ms["first"].sum() == 1 == ms["last"].sum() and ms["first"][0] and ms["last"][-1]
        assert ms["last_word"].sum() == rows - (rows - 1) // 32 * 32 and ms["last_word"][-1] and ms["alternating"].sum() == (rows + 1) // 2
        named = mc.scopes(rows)
        assert {len(v) for v in named.values()} >= {0, 1, 2, 8}
        assert any(not c for v in named.values() for c in v)  # an empty collection
        assert any(s < 0 for v in named.values() for c in v for s, _ in c) and any(e > rows for v in named.values() for c in v for _, e in c)
        dup = mc.range_sets(rows)["duplicates"]
        assert len(dup) > len(set(dup)) and dup != sorted(dup)
        if rows >= 2049:
            assert mc.merged_total(named["lds:exact"], rows) == mc.LDS_RANGES == mc.merged_total(named["lds:exact_in_two"], rows)
            assert mc.merged_total(named["lds:one_more"], rows) == mc.LDS_RANGES + 1 == mc.merged_total(named["lds:one_more_in_two"], rows)
        else:
            assert "lds:exact" not in named
    assert sum(1 for r in mc.ROWS if r >= 2049) >= 4
    assert mc.merge_collection([(5, 9), (1, 3), (3, 4), (8, 12), (20, 20), (-3, 1), (30, 99)], 40) == [(0, 4), (5, 12), (30, 40)]


@pytest.mark.parametrize("rows", mc.ROWS)
def test_the_combine_twin_equals_brute_force(rows):
    for op in mc.OPS.values():
        for n in mc.OPERAND_COUNTS:
            for kind in mc.KINDS:
                ms = mc.operands(kind, n, rows)
                want = _native.pack_mask_bits(mc.combine_bools(op, ms))
                for dirty in (False, True):
                    got = mc.twin_combine_words(op, [mc.pack(m, dirty) for m in ms], rows)
                    assert got.dtype == np.uint32
                    np.testing.assert_array_equal(got, want, err_msg=f"rows {rows} op {op} n {n} {kind} dirty {dirty}")


@pytest.mark.parametrize("rows", mc.ROWS)
def test_the_range_twin_equals_brute_force(rows):
    for name, cols in mc.scopes(rows).items():
        want = mc.range_bool(cols, rows)
        np.testing.assert_array_equal(mc.twin_range_words(cols, rows), _native.pack_mask_bits(want), err_msg=f"rows {rows} {name}")
        # the binding's own helpers: the merged intervals and their union
        for col in cols:
            merged = _native.merge_ranges(_native.range_collections([col])[0], rows)
            assert [tuple(r) for r in merged.tolist()] == mc.merge_collection(col, rows)
            np.testing.assert_array_equal(_native.ranges_to_bool(np.asarray(col, dtype=np.int64).reshape(-1, 2), rows), mc.range_bool([col], rows))
    assert mc.range_bool([], rows).all() and not mc.range_bool([[]], rows).any()


@pytest.mark.parametrize("case", sc.MASK_CASES[::7], ids=[c.name for c in sc.MASK_CASES[::7]])
def test_the_range_twin_over_a_message_map(case):
    m = sc.mask_case_map(case)
    n_messages = int(m[: case.rows].max()) + 1 if (m[: case.rows] >= 0).any() else 0
    for name, cols in mc.message_scopes(case.n_messages, case.seed).items():
        want = mc.range_bool(cols, case.rows, m)
        np.testing.assert_array_equal(mc.twin_range_words(cols, case.rows, m, n_messages), _native.pack_mask_bits(want), err_msg=f"{case.name} {name}")
        # the same scope as enumerated ordinals, through the twin of mask_from_messages_kernel
        ordinals = np.flatnonzero(mc.range_bool(cols, n_messages)) if n_messages else np.zeros(0, np.int64)
        np.testing.assert_array_equal(sc.twin_mask_words(m, case.rows, ordinals, n_messages), _native.pack_mask_bits(want))


# ---- the class on the doubles ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    v, _ = make_corpus(N, D, 9800)
    return v, make_queries(4, D, 9801), sc.message_map(70, N, "interleaved", 9802)


def bools(seed, density=0.5):
    return np.random.default_rng(seed).random(N) < density


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_mask_operators_equal_the_bool_compositions(monkeypatch, corpus, kind):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    A, B, Cm = bools(1), bools(2), bools(3, 0.2)
    a, b, c = vb.row_mask(A), vb.row_mask(B), vb.row_mask(Cm)

    def same(handle, want):
        assert isinstance(handle, RowMask) and handle.rows == N and handle.count == int(want.sum())
        np.testing.assert_array_equal(handle.flat(), np.flatnonzero(want))
        np.testing.assert_array_equal(vb.row_mask(want).flat(), handle.flat())

    same(a & b, A & B)
    same(a | b, A | B)
    same(a - b, A & ~B)
    same(~a, ~A)
    same((a | b) - c, (A | B) & ~Cm)
    same(a & B, A & B)  # anything row_mask accepts
    same(vb.intersect_masks(a, B.tolist(), c), A & B & Cm)
    same(vb.union_masks(a), A)
    same(vb.intersect_masks(a), A)
    many = [bools(10 + i, 0.9) for i in range(19)]  # more than 8 operands: folded in groups
    same(vb.intersect_masks(*many), np.logical_and.reduce(many))
    same(vb.union_masks(*[vb.row_mask(~m) for m in many]), np.logical_or.reduce([~m for m in many]))
    same(a & ~a, np.zeros(N, dtype=bool))
    # the result searches like the bool array it stands for
    want = vb.fuzzy_lookup_embeddings_masked(qs, (A | B) & ~Cm, 10, 0.0)
    assert [pairs(x) for x in vb.fuzzy_lookup_embeddings_masked(qs, (a | b) - c, 10, 0.0)] == [pairs(x) for x in want]


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_range_mask_equals_its_definition(monkeypatch, corpus, kind):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    for name, cols in mc.scopes(N).items():
        want = np.logical_and.reduce([np.ones(N, dtype=bool)] + [_native.ranges_to_bool(np.asarray(c, dtype=np.int64).reshape(-1, 2), N) for c in cols])
        np.testing.assert_array_equal(want, mc.range_bool(cols, N))
        for given in (cols, [np.asarray(c, dtype=np.int64).reshape(-1, 2) for c in cols], tuple(tuple(c) for c in cols)):
            handle = vb.range_mask(given)
            assert isinstance(handle, RowMask) and handle.count == int(want.sum()), name
            np.testing.assert_array_equal(handle.flat(), np.flatnonzero(want), err_msg=name)
    eleven = [[(0, N - i)] for i in range(11)]  # more than 8 collections
    np.testing.assert_array_equal(vb.range_mask(eleven).flat(), np.arange(N - 10))
    vb.set_row_messages(np.concatenate([rm, [5, 6, 7]]))  # a map longer than the index
    n_messages = int(rm.max()) + 1
    for name, cols in mc.message_scopes(n_messages, 9803).items():
        want = rm >= 0
        for c in cols:
            want = want & np.isin(rm, np.flatnonzero(mc.range_bool([c], n_messages)))
        np.testing.assert_array_equal(want, mc.range_bool(cols, N, rm))
        handle = vb.range_mask(cols, of="messages")
        np.testing.assert_array_equal(handle.flat(), np.flatnonzero(want), err_msg=name)
        ordinals = np.flatnonzero(mc.range_bool(cols, n_messages))
        np.testing.assert_array_equal(vb.message_mask(ordinals).flat(), handle.flat())


def test_argument_errors(monkeypatch, corpus):
    v, qs, rm = corpus
    vb = single(monkeypatch, v)
    other = single(monkeypatch, v)
    a = vb.row_mask(bools(1))
    foreign = other.row_mask(bools(2))
    for call in (lambda: a & foreign, lambda: a | foreign, lambda: a - foreign, lambda: vb.intersect_masks(a, foreign), lambda: vb.union_masks(foreign)):
        with pytest.raises(ValueError, match="another index"):
            call()
    with pytest.raises(ValueError, match="at least one mask"):
        vb.intersect_masks()
    with pytest.raises(ValueError, match=f"mask covers {N - 1} rows, the index has {N}"):
        a & bools(1)[:-1]
    with pytest.raises(TypeError, match="must be bool"):
        a | np.arange(N)
    with pytest.raises(ValueError, match='"rows" or "messages"'):
        vb.range_mask([[(0, 3)]], of="chunks")
    with pytest.raises(RuntimeError, match="set_row_messages"):
        vb.range_mask([[(0, 3)]], of="messages")
    with pytest.raises(ValueError, match="pairs"):
        vb.range_mask([[(0, 3, 4)]])
    with pytest.raises(TypeError, match="integers"):
        vb.range_mask([[(0.5, 3.0)]])
    vb.set_row_messages(rm[: N - 1])
    with pytest.raises(ValueError, match=f"covers {N - 1} rows, the index has {N}"):
        vb.range_mask([[(0, 3)]], of="messages")
    vb.add_embeddings(None, v[:1])
    for call in (lambda: ~a, lambda: a & a, lambda: vb.union_masks(a)):
        with pytest.raises(ValueError, match=f"mask covers {N} rows, the index has {N + 1}"):
            call()
    del other
    import gc

    gc.collect()
    with pytest.raises(ValueError, match="is gone"):
        ~foreign


# ---- adapters: the reference's own scope objects -----------------------------------------------------------------------------------------

@dataclass(order=True)
class TextLocation:  # knowpro/interfaces_core.py:223-232 without pydantic
    message_ordinal: int
    chunk_ordinal: int = 0


def _between(text: str, start: str, end: str) -> str:
    i = text.index(start)
    return text[i : text.index(end, i)]


def load_reference_scopes() -> types.SimpleNamespace:
    """The reference's own `TextRange` (knowpro/interfaces_core.py) and `TextRangeCollection` / `TextRangesInScope`
    (knowpro/collections.py), their source lines executed verbatim (the files around them need Python 3.12 and pydantic) over the
    stand-in `TextLocation` above and the standard library's `dataclass`."""
    import bisect
    from collections.abc import Iterable, Iterator

    src = os.path.join(ref_loader.REFERENCE_ROOT, "src", "typeagent", "knowpro")
    ns: dict = {"dataclass": dataclass, "bisect": bisect, "Iterable": Iterable, "Iterator": Iterator, "TextLocation": TextLocation}
    core = open(os.path.join(src, "interfaces_core.py"), encoding="utf-8").read()
    exec(compile("from __future__ import annotations\n" + _between(core, "@dataclass\nclass TextRange:", "    def serialize(self) -> TextRangeData:"),
                 "interfaces_core.py", "exec"), ns)
    coll = open(os.path.join(src, "collections.py"), encoding="utf-8").read()
    exec(compile("from __future__ import annotations\n" + _between(coll, "@dataclass\nclass TextRangeCollection", "@dataclass\nclass TermSet"),
                 "collections.py", "exec"), ns)
    return types.SimpleNamespace(TextLocation=TextLocation, TextRange=ns["TextRange"], TextRangeCollection=ns["TextRangeCollection"],
                                 TextRangesInScope=ns["TextRangesInScope"])


needs_reference = pytest.mark.skipif(not ref_loader.reference_available(), reason="needs the reference checkout (build container only)")


def random_collection(ref, rng, n_messages: int, n_ranges: int):
    ranges = []
    for _ in range(n_ranges):
        m, c = int(rng.integers(0, n_messages)), int(rng.choice([0, 0, 0, 1, 3]))
        shape = rng.integers(0, 4)
        if shape == 0:  # a point
            ranges.append(ref.TextRange(ref.TextLocation(m, c)))
        elif shape == 1:  # an empty or backwards range
            ranges.append(ref.TextRange(ref.TextLocation(m, c), ref.TextLocation(m - int(rng.integers(0, 3)), 0)))
        else:  # a span of some length, either end at a chunk offset
            ranges.append(ref.TextRange(ref.TextLocation(m, c), ref.TextLocation(m + int(rng.integers(0, n_messages // 3)), int(rng.choice([0, 0, 1, 2])))))
    return ref.TextRangeCollection(ranges, ensure_sorted=True)  # (`contains_range` bisects: the reference keeps its collections sorted)


@needs_reference
def test_scope_collections_agree_with_the_reference():
    ref = load_reference_scopes()
    n_messages = 300
    rng = np.random.default_rng(9810)
    seen_in = seen_out = 0
    for trial in range(40):
        scope = ref.TextRangesInScope()
        for _ in range(int(rng.integers(0, 4))):
            scope.add_text_ranges(random_collection(ref, rng, n_messages, int(rng.integers(0, 9))))
        cols = adapters.scope_collections(scope)
        assert len(cols) == (0 if scope.text_ranges is None else len(scope.text_ranges))
        members = mc.range_bool(cols, n_messages)
        for m in range(n_messages):
            want = scope.is_range_in_scope(ref.TextRange(ref.TextLocation(m, 0)))
            assert bool(members[m]) == want, (trial, m, scope)
            seen_in += want
            seen_out += not want
    assert seen_in > 500 and seen_out > 500
    # the other accepted shapes
    one = random_collection(ref, rng, n_messages, 6)
    assert adapters.scope_collections(one) == adapters.scope_collections([one]) == [[adapters._message_range(r) for r in one.get_ranges()]]
    both = ref.TextRangesInScope([one, one])
    assert adapters.scope_collections([both, one]) == adapters.scope_collections(one) * 3
    assert adapters.scope_collections(ref.TextRangesInScope()) == [] and adapters.scope_collections(ref.TextRangeCollection()) == [[]]
    assert adapters.is_text_scope(both) and adapters.is_text_scope(one) and adapters.is_text_scope([one, both])
    assert not adapters.is_text_scope([1, 2]) and not adapters.is_text_scope([]) and not adapters.is_text_scope({3})


# duck-typed stand-ins of the reference's scope objects, for the lookups (no reference needed)
@dataclass
class _Range:
    start: TextLocation
    end: TextLocation | None = None


class _Collection:
    def __init__(self, ranges):
        self._ranges = list(ranges)

    def get_ranges(self):
        return self._ranges


@dataclass
class _Scope:
    text_ranges: list | None = None


def test_the_point_and_offset_rules():
    r = adapters._message_range
    assert r(_Range(TextLocation(4, 0))) == (4, 5) and r(_Range(TextLocation(4, 2)))[0] >= r(_Range(TextLocation(4, 2)))[1]
    assert r(_Range(TextLocation(4, 0), TextLocation(9, 0))) == (4, 9) and r(_Range(TextLocation(4, 1), TextLocation(9, 0))) == (5, 9)
    assert r(_Range(TextLocation(4, 0), TextLocation(9, 3))) == (4, 10) and r(_Range(TextLocation(4, 5), TextLocation(9, 1))) == (5, 10)
    with pytest.raises(TypeError, match="TextRangesInScope or a TextRangeCollection"):
        adapters.scope_collections([_Collection([]), 5])


@pytest.mark.parametrize("kind", list(BUILDERS))
def test_lookup_messages_in_scope_takes_a_text_scope(monkeypatch, corpus, kind):
    v, qs, rm = corpus
    vb = BUILDERS[kind](monkeypatch, v)
    n_messages = int(rm.max()) + 1
    first = _Collection([_Range(TextLocation(3, 0), TextLocation(40, 0)), _Range(TextLocation(50, 0)), _Range(TextLocation(60, 1), TextLocation(66, 2))])
    second = _Collection([_Range(TextLocation(20, 0), TextLocation(n_messages + 5, 0))])
    scope = _Scope([first, second])
    ordinals = np.intersect1d(np.r_[3:40, 50, 61:67], np.arange(20, n_messages))
    np.testing.assert_array_equal(np.flatnonzero(mc.range_bool(adapters.scope_collections(scope), n_messages)), ordinals)
    for max_matches in (None, 3):
        want = adapters.lookup_messages_in_scope(vb, qs, rm, ordinals.tolist(), max_matches, 0.0)
        assert any(want)
        for given in (scope, [first, second], [_Scope([first]), second]):
            got = adapters.lookup_messages_in_scope(vb, qs, rm, given, max_matches, 0.0)
            assert [pairs(x) for x in got] == [pairs(x) for x in want]
        assert pairs(adapters.lookup_messages_in_scope(vb, qs[1], rm, scope, max_matches, 0.0)) == pairs(want[1])
    everything = adapters.lookup_messages_in_scope(vb, qs, rm, _Scope(None), 5, 0.0)
    assert [pairs(x) for x in everything] == [pairs(x) for x in adapters.lookup_messages_in_scope(vb, qs, rm, list(range(n_messages)), 5, 0.0)]
    assert adapters.lookup_messages_in_scope(vb, qs, rm, _Collection([]), 5, 0.0) == [[] for _ in qs]


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_the_abi_is_additive():
    header = open(os.path.join(ROOT, "include", "tavb.h")).read()
    assert int(re.search(r"#define TAVB_ABI_VERSION (\d+)", header).group(1)) == 7 == _native.ABI_VERSION
    assert int(re.search(r"#define TAVB_KERNEL_COUNT (\d+)", header).group(1)) == 10
    for name, value in (("TAVB_MAX_SCOPE_COLLECTIONS", _native.MAX_SCOPE_COLLECTIONS), ("TAVB_MAX_MASK_OPERANDS", _native.MAX_MASK_OPERANDS),
                        ("TAVB_MASK_AND", _native.MASK_AND), ("TAVB_MASK_OR", _native.MASK_OR), ("TAVB_MASK_ANDNOT", _native.MASK_ANDNOT),
                        ("TAVB_SCOPE_LDS_RANGES", _native.SCOPE_LDS_RANGES)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"typedef struct \{\s*int64_t count, first_row, last_row;\s*\} tavb_mask_info;", code)
    lib = _native.load_library(preload_torch=False)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\s*\(tavb_ctx\* ctx,", code), f"{name} is not declared in include/tavb.h"
        assert name in _native.ABI_SYMBOLS and hasattr(lib, name)
    # without a context both fail cleanly, whatever else they are handed: the context is looked at first
    import ctypes

    info = _native.MaskInfo(7, 7, 7)
    assert lib.tavb_mask_from_ranges(None, None, None, 0, 0, 0, None, None, 0, ctypes.byref(info)) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_mask_from_ranges(None, None, None, 9, 2, -1, None, None, -1, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_mask_combine(None, 0, None, 1, 0, None, None, 0, ctypes.byref(info)) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_mask_combine(None, 3, None, 9, -1, None, None, -1, None) == -1 and b"null context" in lib.tavb_last_error()
    assert (info.count, info.first_row, info.last_row) == (7, 7, 7)
    for method in ("mask_from_ranges", "mask_combine"):
        assert callable(getattr(_native.Engine, method))
    for method in ("intersect_masks", "union_masks", "range_mask"):
        assert callable(getattr(VectorBase, method))
    for method in ("__and__", "__or__", "__sub__", "__invert__"):
        assert callable(getattr(RowMask, method))
    assert callable(adapters.scope_collections)
