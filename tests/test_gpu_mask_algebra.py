"""GPU suite: the scope algebra -- `mask_combine_kernel` behind tavb_mask_combine, `mask_from_ranges_kernel` behind tavb_mask_from_ranges,
and `RowMask`'s operators, `VectorBase.range_mask` and `adapters.lookup_messages_in_scope` on top of them.  The table is
tests/mask_algebra_cases.py; tests/test_mask_algebra_host.py pins it on the CPU.

  1. tavb_mask_combine at every row count x op x operand count x operand kind: words (whole, tail bits zero, the word behind the mask
     untouched), count, first, last and the row list against numpy -- with clean operands and with every bit at or beyond `rows` set; the
     output aliasing operand 0 and operand n - 1; a capacity one short of the count; an empty result; the argument errors;
  2. tavb_mask_from_ranges over rows at the same row counts for every scope of the table (0, 1, 2 and 8 collections; both sides of
     TAVB_SCOPE_LDS_RANGES), and over the message maps of tests/message_scope_cases.py, where it equals the words of
     tavb_mask_from_messages over the host-enumerated ordinals;
  3. end to end on the 3000-row corpora of tests/message_scope_cases.py: `a & b` and `(a | b) - c` search like the row list of the same
     expression (route 1, bit for bit) and like `row_mask(bool array)` on the forced tile routes (bit for bit: the words are identical);
     `lookup_messages_in_scope` with a two-collection scope equals the host-intersected ordinal list."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

from tests import mask_algebra_cases as mc
from tests import message_scope_cases as sc
from tests.test_mask_algebra_host import TextLocation, _Collection, _Range, _Scope
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native, adapters

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def bits32(hits):
    return [(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits]


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine(0)
    yield e
    e.close()


def set_rows(eng, rows: int) -> None:
    eng.set_corpus_tensor(_torch().zeros((rows, 8), dtype=_torch().float32, device="cuda"))


def dev(words: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(words).view(np.int32)).cuda()


def info_of(flat: np.ndarray):
    return (len(flat), int(flat[0]), int(flat[-1])) if len(flat) else (0, 0, -1)


def raw_combine(eng, op, tensors, rows, out, rows_out=None, cap=0):
    """tavb_mask_combine itself -> (rc, (count, first, last))."""
    ptrs = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    info = _native.MaskInfo(-5, -5, -5)
    _torch().cuda.synchronize()
    rc = eng.lib.tavb_mask_combine(eng._h, op, ptrs, len(tensors), rows, ctypes.c_void_p(out.data_ptr()),
                                   None if rows_out is None else ctypes.c_void_p(rows_out.data_ptr()), cap, ctypes.byref(info))
    return rc, (info.count, info.first_row, info.last_row)


def raw_ranges(eng, cols, domain, rows, out, rows_out=None, cap=0):
    arrays = _native.range_collections(cols)
    ranges = np.ascontiguousarray(np.concatenate(arrays)) if arrays else np.zeros((0, 2), dtype=np.int64)
    sizes = np.array([len(a) for a in arrays], dtype=np.int32)
    info = _native.MaskInfo(-5, -5, -5)
    _torch().cuda.synchronize()
    rc = eng.lib.tavb_mask_from_ranges(eng._h, _native._addr(ranges) if ranges.size else None, _native._addr(sizes) if sizes.size else None, len(arrays), domain,
                                       rows, ctypes.c_void_p(out.data_ptr()), None if rows_out is None else ctypes.c_void_p(rows_out.data_ptr()), cap,
                                       ctypes.byref(info))
    return rc, (info.count, info.first_row, info.last_row)


# ---- 1. tavb_mask_combine ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", mc.ROWS)
def test_combine(eng, rows):
    torch = _torch()
    set_rows(eng, rows)
    n_words = (rows + 31) // 32
    for opname, op in mc.OPS.items():
        for n in mc.OPERAND_COUNTS:
            for kind in mc.KINDS:
                ms = mc.operands(kind, n, rows)
                want_bool = mc.combine_bools(op, ms)
                want = _native.pack_mask_bits(want_bool)
                flat = np.flatnonzero(want_bool)
                tag = f"rows {rows} {opname} n {n} {kind}"
                for dirty in (False, True):
                    tensors = [dev(mc.pack(m, dirty)) for m in ms]
                    out = torch.full((n_words + 1,), -1, dtype=torch.int32, device="cuda")
                    rows_out = torch.full((len(flat) + 1,), -7, dtype=torch.int32, device="cuda")
                    rc, info = raw_combine(eng, op, tensors, rows, out, rows_out, len(flat))
                    assert rc == 0, eng.lib.tavb_last_error()
                    got = out.cpu().numpy().view(np.uint32)
                    assert got[n_words] == 0xFFFFFFFF, f"{tag}: the word behind the mask was written"
                    np.testing.assert_array_equal(got[:n_words], want, err_msg=tag)
                    assert info == info_of(flat), tag
                    listed = rows_out.cpu().numpy()
                    np.testing.assert_array_equal(listed[: len(flat)], flat.astype(np.int32), err_msg=tag)
                    assert listed[len(flat)] == -7, f"{tag}: the list was written beyond the count"
                # the output over operand 0 and over operand n - 1 (dirty operands)
                for where in {0, n - 1}:
                    tensors = [dev(mc.pack(m, True)) for m in ms]
                    rc, info = raw_combine(eng, op, tensors, rows, tensors[where])
                    assert rc == 0 and info == info_of(flat), tag
                    got = tensors[where].cpu().numpy().view(np.uint32)
                    np.testing.assert_array_equal(got[:n_words], want, err_msg=f"{tag} in place over operand {where}")
                    assert got[n_words] == 0xFFFFFFFF
                # the binding
                dev_rows, count, dev_bits, span = eng.mask_combine(op, [dev(mc.pack(m)) for m in ms], rows)
                assert (count, span) == (len(flat), (int(flat[0]), int(flat[-1])) if len(flat) else None) and int(dev_rows.numel()) == count
                np.testing.assert_array_equal(dev_bits.cpu().numpy().view(np.uint32), want)
                np.testing.assert_array_equal(dev_rows.cpu().numpy(), flat.astype(np.int32))


def test_combine_capacity_and_argument_errors(eng):
    torch = _torch()
    rows = mc.C + 1
    set_rows(eng, rows)
    n_words = (rows + 31) // 32
    a, b = mc.operand("random0.5", rows, 1), mc.operand("random0.5", rows, 2)
    flat = np.flatnonzero(a | b)
    ta, tb = dev(mc.pack(a)), dev(mc.pack(b))
    out = torch.zeros(n_words + 1, dtype=torch.int32, device="cuda")
    short = torch.full((len(flat),), -7, dtype=torch.int32, device="cuda")
    rc, info = raw_combine(eng, mc.OR, [ta, tb], rows, out, short, len(flat) - 1)  # one short of the count
    assert rc == -1 and b"rows set" in eng.lib.tavb_last_error() and info == info_of(flat)
    listed = short.cpu().numpy()
    np.testing.assert_array_equal(listed[:-1], flat[:-1].astype(np.int32))
    assert listed[-1] == -7, "written at the capacity"
    with pytest.raises(ValueError, match="rows set"):
        eng.mask_combine(mc.OR, [ta, tb], len(flat) - 1)
    rc, info = raw_combine(eng, mc.AND, [ta, dev(mc.pack(~a))], rows, out)  # an empty result, the info alone
    assert rc == 0 and info == (0, 0, -1) and not out.cpu().numpy()[:n_words].any()
    dev_rows, count, _, span = eng.mask_combine(mc.AND, [ta, dev(mc.pack(~a))], 0)
    assert int(dev_rows.numel()) == 0 and count == 0 and span is None
    for op, tensors, r in ((3, [ta], rows), (-1, [ta], rows), (mc.AND, [ta], rows - 1), (mc.AND, [ta] * 9, rows)):
        rc, info = raw_combine(eng, op, tensors, r, out)
        assert rc == -1 and info == (0, 0, -1), (op, len(tensors), r)
    info = _native.MaskInfo()
    ptrs = (ctypes.c_void_p * 2)(ta.data_ptr(), None)
    o = ctypes.c_void_p(out.data_ptr())
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, ptrs, 2, rows, o, None, 0, ctypes.byref(info)) == -1  # a null operand
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, None, 1, rows, o, None, 0, ctypes.byref(info)) == -1
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, ptrs, 1, rows, None, None, 0, ctypes.byref(info)) == -1
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, ptrs, 1, rows, o, None, 5, ctypes.byref(info)) == -1  # a capacity without a list
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, ptrs, 1, rows, o, None, -1, ctypes.byref(info)) == -1
    assert eng.lib.tavb_mask_combine(eng._h, mc.AND, ptrs, 1, rows, o, None, 0, None) == -1
    with pytest.raises(ValueError, match="1 .. 8 operands"):
        eng.mask_combine(mc.AND, [], 0)


# ---- 2. tavb_mask_from_ranges ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", mc.ROWS)
def test_ranges_over_rows(eng, rows):
    torch = _torch()
    set_rows(eng, rows)
    n_words = (rows + 31) // 32
    for name, cols in mc.scopes(rows).items():
        want_bool = mc.range_bool(cols, rows)
        want = mc.twin_range_words(cols, rows)
        flat = np.flatnonzero(want_bool)
        tag = f"rows {rows} {name}"
        out = torch.full((n_words + 1,), -1, dtype=torch.int32, device="cuda")
        rows_out = torch.full((len(flat) + 1,), -7, dtype=torch.int32, device="cuda")
        rc, info = raw_ranges(eng, cols, 0, rows, out, rows_out, len(flat))
        assert rc == 0, eng.lib.tavb_last_error()
        got = out.cpu().numpy().view(np.uint32)
        assert got[n_words] == 0xFFFFFFFF, f"{tag}: the word behind the mask was written"
        np.testing.assert_array_equal(got[:n_words], want, err_msg=tag)
        assert info == info_of(flat), tag
        listed = rows_out.cpu().numpy()
        np.testing.assert_array_equal(listed[: len(flat)], flat.astype(np.int32), err_msg=tag)
        assert listed[len(flat)] == -7
        rc, info = raw_ranges(eng, cols, 0, rows, out)  # the mask and its info only
        assert rc == 0 and info == info_of(flat), tag
        dev_rows, count, dev_bits, span = eng.mask_from_ranges(cols, "rows")
        assert (count, span) == (len(flat), (int(flat[0]), int(flat[-1])) if len(flat) else None) and int(dev_rows.numel()) == count, tag
        np.testing.assert_array_equal(dev_bits.cpu().numpy().view(np.uint32), want, err_msg=tag)
        np.testing.assert_array_equal(dev_rows.cpu().numpy(), flat.astype(np.int32), err_msg=tag)


@pytest.mark.parametrize("case", sc.MASK_CASES, ids=[c.name for c in sc.MASK_CASES])
def test_ranges_over_messages(eng, case):
    torch = _torch()
    m = sc.mask_case_map(case)
    set_rows(eng, case.rows)
    eng.set_row_messages(m)
    n_messages = int(m.max()) + 1 if (m >= 0).any() else 0  # what the binding hands to tavb_set_row_messages
    n_words = (case.rows + 31) // 32
    for name, cols in mc.message_scopes(case.n_messages, case.seed).items():
        tag = f"{case.name} {name}"
        want_bool = mc.range_bool(cols, case.rows, m)
        flat = np.flatnonzero(want_bool)
        ordinals = np.flatnonzero(mc.range_bool(cols, n_messages)) if n_messages else np.zeros(0, np.int64)
        _, _, enumerated = eng.mask_from_messages(ordinals)  # tavb_mask_from_messages over the host-enumerated ordinals
        want = enumerated.cpu().numpy().view(np.uint32)
        np.testing.assert_array_equal(want, _native.pack_mask_bits(want_bool), err_msg=tag)
        np.testing.assert_array_equal(want, mc.twin_range_words(cols, case.rows, m, n_messages), err_msg=tag)
        out = torch.full((n_words + 1,), -1, dtype=torch.int32, device="cuda")
        rc, info = raw_ranges(eng, cols, 1, case.rows, out)
        assert rc == 0, eng.lib.tavb_last_error()
        got = out.cpu().numpy().view(np.uint32)
        assert got[n_words] == 0xFFFFFFFF
        np.testing.assert_array_equal(got[:n_words], want, err_msg=tag)
        assert info == info_of(flat), tag
        dev_rows, count, dev_bits, span = eng.mask_from_ranges(cols, "messages")
        assert (count, span) == (len(flat), (int(flat[0]), int(flat[-1])) if len(flat) else None), tag
        np.testing.assert_array_equal(dev_bits.cpu().numpy().view(np.uint32), want, err_msg=tag)
        np.testing.assert_array_equal(dev_rows.cpu().numpy(), flat.astype(np.int32), err_msg=tag)


def test_ranges_argument_errors():
    torch = _torch()
    eng = _native.Engine(0)
    rows = 100
    set_rows(eng, rows)
    out = torch.zeros(5, dtype=torch.int32, device="cuda")
    with pytest.raises(_native.TavbError, match="no row -> message map"):
        eng.mask_from_ranges([[(0, 5)]], "messages")
    eng.set_row_messages(np.zeros(99, dtype=np.int64))
    with pytest.raises(ValueError, match="covers 99 rows, the corpus has 100"):
        eng.mask_from_ranges([[(0, 5)]], "messages")
    eng.set_row_messages(np.zeros(100, dtype=np.int64))
    assert raw_ranges(eng, [[(0, 5)]], 1, rows, out) == (0, (100, 0, 99))
    for cols, domain, r in (([[(0, 5)]], 2, rows), ([[(0, 5)]], -1, rows), ([[(0, 5)]], 0, rows - 1), ([[(0, 5)]] * 9, 0, rows)):
        rc, info = raw_ranges(eng, cols, domain, r, out)
        assert rc == -1 and info == (0, 0, -1), (len(cols), domain, r)
    info = _native.MaskInfo()
    o = ctypes.c_void_p(out.data_ptr())
    ranges = np.array([[0, 5]], dtype=np.int64)
    call = eng.lib.tavb_mask_from_ranges
    assert call(eng._h, _native._addr(ranges), _native._addr(np.array([-1], dtype=np.int32)), 1, 0, rows, o, None, 0, ctypes.byref(info)) == -1  # a negative size
    assert call(eng._h, _native._addr(ranges), _native._addr(np.array([(1 << 20) + 1], dtype=np.int32)), 1, 0, rows, o, None, 0, ctypes.byref(info)) == -1
    assert b"2^20" in eng.lib.tavb_last_error()
    one = np.array([1], dtype=np.int32)
    assert call(eng._h, None, _native._addr(one), 1, 0, rows, o, None, 0, ctypes.byref(info)) == -1  # ranges without an address
    assert call(eng._h, _native._addr(ranges), None, 1, 0, rows, o, None, 0, ctypes.byref(info)) == -1
    assert call(eng._h, _native._addr(ranges), _native._addr(one), 1, 0, rows, None, None, 0, ctypes.byref(info)) == -1
    assert call(eng._h, _native._addr(ranges), _native._addr(one), 1, 0, rows, o, None, 3, ctypes.byref(info)) == -1
    assert call(eng._h, _native._addr(ranges), _native._addr(one), 1, 0, rows, o, None, 0, None) == -1
    short = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    rc, got = raw_ranges(eng, [[(10, 15)]], 0, rows, out, short, 4)  # one short of the count
    assert rc == -1 and got == (5, 10, 14) and short.cpu().numpy().tolist() == [10, 11, 12, 13, -7]
    with pytest.raises(ValueError, match="at most 8 collections"):
        eng.mask_from_ranges([[(0, 5)]] * 9)
    eng.close()


# ---- 3. end to end -----------------------------------------------------------------------------------------------------------------------

_state: dict = {}


def index(corpus: sc.Corpus):
    if corpus.name not in _state:
        v, _ = make_corpus(sc.ROWS, corpus.dim, corpus.seed)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=corpus.dtype)
        vb.add_embeddings(None, v)
        vb.set_row_messages(sc.lookup_map())
        _state[corpus.name] = (vb, make_queries(65, corpus.dim, corpus.seed + 1))
    return _state[corpus.name]


def force(eng, route: str) -> None:
    tile, wide = sc.ROUTES[route]
    eng.set_option("mask_tile", tile)
    eng.set_option("mask_wide", wide)


def same_arrays(a, b, nq, tag):
    assert np.array_equal(a[2], b[2]), tag
    for q in range(nq):
        m = int(a[2][q])
        assert np.array_equal(a[0][q, :m], b[0][q, :m]) and np.array_equal(a[1][q, :m].view(np.uint32), b[1][q, :m].view(np.uint32)), (tag, q)


@pytest.mark.parametrize("corpus", sc.CORPORA[:2], ids=[c.name for c in sc.CORPORA[:2]])
def test_expressions_search_like_their_bool_arrays(corpus):
    vb, qs = index(corpus)
    eng = vb.engine
    rng = np.random.default_rng(9900)
    A, B, Cm = rng.random(sc.ROWS) < 0.6, rng.random(sc.ROWS) < 0.5, rng.random(sc.ROWS) < 0.2
    a, b, c = vb.row_mask(A), vb.row_mask(B), vb.row_mask(Cm)
    for expr, want_bool in ((lambda: a & b, A & B), (lambda: (a | b) - c, (A | B) & ~Cm)):
        handle = expr()
        flat = np.flatnonzero(want_bool)
        assert isinstance(handle, RowMask) and handle.count == len(flat) and handle.span == (int(flat[0]), int(flat[-1]))
        assert handle.dev_rows is not None and handle.dev_bits is not None
        np.testing.assert_array_equal(handle.dev_rows.cpu().numpy(), flat.astype(np.int32))
        np.testing.assert_array_equal(handle.dev_bits.cpu().numpy().view(np.uint32), _native.pack_mask_bits(want_bool))
        try:
            for nq in (1, 9, 65):
                force(eng, "list")
                got = vb.fuzzy_lookup_embeddings_masked(qs[:nq], handle, 10, 0.5)
                assert eng.get_option("masked_route") == 1
                for i in range(nq):
                    assert bits32(got[i]) == bits32(vb.fuzzy_lookup_embedding_in_subset(qs[i], flat.tolist(), 10, 0.5)), (nq, i)
                for route in ("tile", "wide"):
                    force(eng, route)
                    x = vb.fuzzy_lookup_embeddings_masked(qs[:nq], handle, 10, 0.5, as_arrays=True)
                    rx = eng.get_option("masked_route")
                    y = vb.fuzzy_lookup_embeddings_masked(qs[:nq], vb.row_mask(want_bool), 10, 0.5, as_arrays=True)
                    assert rx == eng.get_option("masked_route")
                    assert rx == (1 if route == "wide" and corpus.dtype == "float32" else {"tile": 2, "wide": 3}[route])
                    same_arrays(x, y, nq, (route, nq))
        finally:
            eng.set_option("mask_tile", 1)
            eng.set_option("mask_wide", 1)
    assert (~a).count == sc.ROWS - a.count and (a & ~a).count == 0 and (a & ~a).span is None
    np.testing.assert_array_equal(vb.range_mask([[(100, 2000)], [(50, 150), (1900, 5000)]]).flat(), np.r_[100:150, 1900:2000])
    np.testing.assert_array_equal(vb.intersect_masks(*[vb.range_mask([[(i, 3000 - i)]]) for i in range(11)]).flat(), np.arange(10, 2990))
    # a handle of another index, or of another length
    other, _ = index(sc.CORPORA[1] if corpus is sc.CORPORA[0] else sc.CORPORA[0])
    with pytest.raises(ValueError, match="another index"):
        a & other.row_mask(A)
    with pytest.raises(ValueError, match="mask covers 2999 rows, the index has 3000"):
        a | A[:-1]


def test_lookup_messages_in_scope_with_a_text_scope():
    vb, qs = index(sc.CORPORA[0])
    rm = sc.lookup_map()
    first = _Collection([_Range(TextLocation(100, 0), TextLocation(700, 0)), _Range(TextLocation(900, 0)), _Range(TextLocation(950, 2), TextLocation(960, 1))])
    second = _Collection([_Range(TextLocation(400, 0), TextLocation(5000, 0)), _Range(TextLocation(3, 0), TextLocation(3, 1))])
    scope = _Scope([first, second])
    ordinals = np.intersect1d(np.r_[100:700, 900, 951:961], np.r_[400:1000, 3])  # the host route this replaces
    handle = vb.range_mask(adapters.scope_collections(scope), of="messages")
    np.testing.assert_array_equal(handle.flat(), np.flatnonzero(sc.isin_mask(rm, sc.ROWS, ordinals)))
    assert handle.dev_bits is not None and handle.span == (int(handle.flat()[0]), int(handle.flat()[-1]))
    for max_matches in (None, 5, 40):
        want = adapters.lookup_messages_in_scope(vb, qs[:9], rm, ordinals.tolist(), max_matches, 0.5)
        got = adapters.lookup_messages_in_scope(vb, qs[:9], rm, scope, max_matches, 0.5)
        assert [bits32(x) for x in got] == [bits32(x) for x in want] and any(want)
        assert bits32(adapters.lookup_messages_in_scope(vb, qs[3], rm, [first, second], max_matches, 0.5)) == bits32(want[3])
