"""CPU suite: what `_native.Engine`'s batched and subset methods hand to the library -- the symbol, the argument count of its prototype, the
integer arguments, the thresholds array, the shapes and dtypes that come back -- over a recording stand-in for `lib` on an Engine that never
reaches libtavb.so.  The device-query and merge forms are reached as far as a host can go: their refusals."""

from __future__ import annotations

import ctypes
import threading

import numpy as np
import pytest

from typeagent_py_amd import _native

torch = pytest.importorskip("torch")

ROWS, DIM, NQ, K = 512, 8, 3, 5
ARGC = {name: len(argtypes) for name, _, argtypes in _native._SIGNATURES}


class _RecordingLib:
    """`tavb_*` attributes record (symbol, args) and return 0; `counts[symbol]` is written through the call's last (byref) argument first."""

    def __init__(self, counts=None):
        self.calls = []
        self.counts = counts or {}

    def __getattr__(self, name):
        if not name.startswith("tavb_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if name in self.counts:
                args[-1]._obj.value = self.counts[name]
            return 0

        return call


def _engine(counts=None, ordinal_base=0):
    eng = _native.Engine.__new__(_native.Engine)
    eng._torch, eng.device, eng.dim, eng.rows, eng.dtype, eng.ordinal_base = torch, 0, DIM, ROWS, _native.TAVB_F16, ordinal_base
    eng._h, eng._lock, eng._out_cache = ctypes.c_void_p(0x1000), threading.Lock(), {}
    eng.lib = _RecordingLib(counts)
    return eng


def _ptr(arg):
    if arg is None:
        return None
    return arg.value if isinstance(arg, ctypes.c_void_p) else ctypes.addressof(arg)


def _floats(arg, n):
    return np.ctypeslib.as_array((ctypes.c_float * n).from_address(_ptr(arg))).copy()


def _one_call(eng, symbol):
    assert [name for name, _ in eng.lib.calls] == [symbol]
    args = eng.lib.calls[0][1]
    assert len(args) == ARGC[symbol], f"{symbol}: {len(args)} arguments for a prototype of {ARGC[symbol]}"
    assert args[0] is eng._h
    return args


def _queries(nq=NQ):
    return np.arange(nq * DIM, dtype=np.float64).reshape(nq, DIM)[:, ::-1] / 7.0  # float64 and strided: the binding makes it float32, contiguous


def _bits():
    return torch.zeros((ROWS + 31) // 32, dtype=torch.int32)


def _rows(n=171):
    return torch.arange(0, 3 * n, 3, dtype=torch.int32)  # every third row


THRS = [np.float32(0.25), np.array([0.1, 0.2, 0.3], dtype=np.float32), [0.5, 0.25, 0.125], np.array([0.75])]


def _check_batch(eng, symbol, out, queries, thrs, at, ints, k=K, out_dtypes=(np.int64, np.float32, np.int32)):
    """`at`: positions of (queries, nq, thresholds) in the call; `ints`: {position: value} of the other integer arguments."""
    args = _one_call(eng, symbol)
    nq = len(queries)
    np.testing.assert_array_equal(_floats(args[at[0]], nq * DIM).reshape(nq, DIM), queries.astype(np.float32))
    assert args[at[1]] == nq and type(args[at[1]]) is int
    np.testing.assert_array_equal(_floats(args[at[2]], nq), np.broadcast_to(np.asarray(thrs, dtype=np.float32), (nq,)))
    for pos, want in ints.items():
        assert args[pos] == want and type(args[pos]) is int, f"{symbol}: argument {pos} is {args[pos]!r}, not {want!r}"
    ords, scs, cnts = out
    assert ords.shape == scs.shape == (nq, k) and cnts.shape == (nq,)
    assert (ords.dtype, scs.dtype, cnts.dtype) == out_dtypes
    assert not cnts.any()
    for arr, pos in zip(out, range(len(args) - 3, len(args))):
        assert _ptr(args[pos]) == arr.ctypes.data  # the arrays that come back are the ones the library wrote
    return args


@pytest.mark.parametrize("thrs", THRS, ids=["scalar", "array", "list", "one"])
def test_search_batch_and_topk(thrs):
    for method, symbol in (("search_batch", "tavb_search_batch"), ("search_topk", "tavb_search_topk")):
        eng, q = _engine(), _queries()
        _check_batch(eng, symbol, getattr(eng, method)(q, K, thrs), q, thrs, (1, 2, 4), {3: K})


@pytest.mark.parametrize("span,first,last", [(None, 0, ROWS - 1), ((3, 400), 3, 400)])
def test_search_masked_batch(span, first, last):
    eng, q, bits = _engine(), _queries(), _bits()
    args = _check_batch(eng, "tavb_search_masked_batch", eng.search_masked_batch(q, bits, K, THRS[1], span=span), q, THRS[1], (1, 2, 8),
                        {4: ROWS, 5: first, 6: last, 7: K})
    assert _ptr(args[3]) == bits.data_ptr()


@pytest.mark.parametrize("n_allowed", [171, 0])
def test_search_masked_wide(n_allowed):
    eng, q, bits, rows = _engine(), _queries(), _bits(), _rows(n_allowed)
    args = _check_batch(eng, "tavb_search_masked_wide", eng.search_masked_wide(q, bits, rows, K, 0.5, span=(0, 510)), q, 0.5, (1, 2, 10),
                        {4: ROWS, 5: 0, 6: 510, 8: n_allowed, 9: K})
    assert _ptr(args[3]) == bits.data_ptr()
    assert _ptr(args[7]) == (rows.data_ptr() if n_allowed else None)  # an empty list goes as (no pointer, 0)


@pytest.mark.parametrize("remap", [True, False])
@pytest.mark.parametrize("n_allowed", [171, 0])
def test_search_subset_batch_resident(n_allowed, remap):
    eng, q, rows = _engine(), _queries(), _rows(n_allowed)
    args = _check_batch(eng, "tavb_search_subset_batch_resident", eng.search_subset_batch_resident(q, rows, K, THRS[2], remap=remap), q, THRS[2],
                        (1, 2, 6), {4: n_allowed, 5: K, 7: int(remap)})
    assert _ptr(args[3]) == (rows.data_ptr() if n_allowed else None)


@pytest.mark.parametrize("k,bound", [(0, NQ * ROWS), (7, NQ * 7), (ROWS + 9, NQ * ROWS)])
def test_search_sorted(k, bound):
    eng, q = _engine(counts={"tavb_search_sorted": 4}), _queries()
    ords, scs, cnts = eng.search_sorted(q, k, THRS[1])
    args = _one_call(eng, "tavb_search_sorted")
    np.testing.assert_array_equal(_floats(args[1], NQ * DIM).reshape(NQ, DIM), q.astype(np.float32))
    assert (args[2], args[3], args[5]) == (NQ, k, bound)
    np.testing.assert_array_equal(_floats(args[4], NQ), THRS[1])
    assert ords.shape == scs.shape == (4,) and (ords.dtype, scs.dtype) == (np.int64, np.float32)  # the first `total` of bound-sized outputs
    assert ords.base.shape == scs.base.shape == (bound,)
    assert cnts.shape == (NQ,) and cnts.dtype == np.int64 and not cnts.any()
    with pytest.raises(ValueError, match="k must be >= 0"):
        _engine().search_sorted(q, -1, 0.5)


@pytest.mark.parametrize("route", [1, 2, 3])
def test_search_messages_masked(route):
    eng, q, bits, rows = _engine(), _queries(), _bits(), _rows()
    args = _check_batch(eng, "tavb_search_messages_masked", eng.search_messages_masked(q, bits, rows, K, THRS[1], 4, route, span=(0, 510)), q, THRS[1],
                        (1, 2, 10), {4: ROWS, 5: 0, 6: 510, 8: 171, 9: K, 11: 4, 12: route})
    assert (_ptr(args[3]), _ptr(args[7])) == (bits.data_ptr(), rows.data_ptr())
    eng = _engine()
    eng.search_messages_masked(q, bits, None, K, 0.5, 4, 2)  # the tile route needs no row list
    args = _one_call(eng, "tavb_search_messages_masked")
    assert (args[5], args[6], args[7], args[8]) == (0, ROWS - 1, None, 0)


@pytest.mark.parametrize("accept,n_accept", [(None, -1), ([4, 9, 2], 3), ([], 0)])
def test_search_messages_batch(accept, n_accept):
    eng, q = _engine(), _queries()
    args = _check_batch(eng, "tavb_search_messages_batch", eng.search_messages_batch(q, K, THRS[0], 4, accept=accept), q, THRS[0], (1, 2, 4),
                        {3: K, 6: n_accept, 7: 4})
    if n_accept > 0:
        np.testing.assert_array_equal(np.ctypeslib.as_array((ctypes.c_int32 * n_accept).from_address(_ptr(args[5]))), accept)
    else:
        assert args[5] is None


HOST_BATCH = [
    ("tavb_search_batch", lambda e, q: e.search_batch(q, K, 0.5)),
    ("tavb_search_topk", lambda e, q: e.search_topk(q, K, 0.5)),
    ("tavb_search_sorted", lambda e, q: e.search_sorted(q, K, 0.5)),
    ("tavb_search_masked_batch", lambda e, q: e.search_masked_batch(q, _bits(), K, 0.5)),
    ("tavb_search_masked_wide", lambda e, q: e.search_masked_wide(q, _bits(), _rows(), K, 0.5)),
    ("tavb_search_subset_batch_resident", lambda e, q: e.search_subset_batch_resident(q, _rows(), K, 0.5)),
    ("tavb_search_messages_masked", lambda e, q: e.search_messages_masked(q, _bits(), _rows(), K, 0.5, 4, 1)),
    ("tavb_search_messages_batch", lambda e, q: e.search_messages_batch(q, K, 0.5, 4)),
]


@pytest.mark.parametrize("symbol,call", HOST_BATCH, ids=[s for s, _ in HOST_BATCH])
def test_host_batch_refuses_wrong_shape_queries(symbol, call):
    for bad in (np.zeros((NQ, DIM + 1), np.float32), np.zeros(DIM, np.float32), np.zeros((1, NQ, DIM), np.float32)):
        eng = _engine()
        with pytest.raises(ValueError, match=rf"^queries must be \[nq, {DIM}\]$"):
            call(eng, bad)
        assert eng.lib.calls == []
    eng = _engine()
    call(eng, np.zeros((0, DIM), np.float32))  # an empty batch is not refused here: the library answers it
    assert eng.lib.calls[0][0] == symbol and eng.lib.calls[0][1][2] == 0


# ---- one query over a subset -------------------------------------------------------------------------------------------------------------

def _check_single(eng, symbol, out, q, at_query, ints, thr_at, m=2, k=K):
    args = _one_call(eng, symbol)
    np.testing.assert_array_equal(_floats(args[at_query], DIM), q.astype(np.float32))
    for pos, want in ints.items():
        assert args[pos] == want, f"{symbol}: argument {pos} is {args[pos]!r}, not {want!r}"
    assert isinstance(args[thr_at], ctypes.c_float) and args[thr_at].value == np.float32(0.3)
    pos, scs = out
    assert pos.shape == scs.shape == (m,) and (pos.dtype, scs.dtype) == (np.int64, np.float32)  # the first `count` of k-sized outputs
    assert pos.base.shape == scs.base.shape == (k,)
    assert (_ptr(args[-3]), _ptr(args[-2])) == (pos.ctypes.data, scs.ctypes.data)
    assert isinstance(args[-1]._obj, ctypes.c_int32)
    return args


def _query():
    return np.arange(DIM, dtype=np.float64)[::-1] / 3.0


SUBSET = np.array([5, 500, 17, 2], dtype=np.int32)


def test_search_subset_and_topk():
    for method, symbol in (("search_subset", "tavb_search_subset"), ("search_subset_topk", "tavb_search_subset_topk")):
        eng, q = _engine(counts={symbol: 2}), _query()
        args = _check_single(eng, symbol, getattr(eng, method)(q, SUBSET, K, np.float32(0.3)), q, 1, {3: 4, 4: K}, 5)
        np.testing.assert_array_equal(np.ctypeslib.as_array((ctypes.c_int64 * 4).from_address(_ptr(args[2]))), SUBSET)


def test_search_subset_after():
    eng, q = _engine(counts={"tavb_search_subset_after": 2}), _query()
    args = _check_single(eng, "tavb_search_subset_after", eng.search_subset(q, SUBSET, K, np.float32(0.3), after=(0.5, 17)), q, 1, {3: 4, 4: K, 7: 17}, 5)
    assert args[6].value == 0.5


@pytest.mark.parametrize("n", [171, 0])
def test_search_subset_resident(n):
    eng, q, rows = _engine(counts={"tavb_search_subset_resident": 2}), _query(), _rows(n)
    args = _check_single(eng, "tavb_search_subset_resident", eng.search_subset_resident(q, rows, K, np.float32(0.3)), q, 1, {3: n, 4: K}, 5)
    assert isinstance(args[2], ctypes.c_void_p) and (args[2].value or 0) == rows.data_ptr()  # the pointer goes unconditionally


def test_search_messages():
    eng, q = _engine(counts={"tavb_search_messages": 2}), _query()
    args = _check_single(eng, "tavb_search_messages", eng.search_messages(q, K, np.float32(0.3), 4, accept=[7, 1]), q, 1, {2: K, 5: 2, 6: 4}, 3)
    np.testing.assert_array_equal(np.ctypeslib.as_array((ctypes.c_int32 * 2).from_address(_ptr(args[4]))), [7, 1])
    for accept, n_accept in ((None, -1), ([], 0)):
        eng = _engine(counts={"tavb_search_messages": 2})
        args = _check_single(eng, "tavb_search_messages", eng.search_messages(q, K, np.float32(0.3), 4, accept=accept), q, 1, {2: K, 4: None, 5: n_accept, 6: 4}, 3)
    eng = _engine(counts={"tavb_search_messages_subset": 2})
    args = _check_single(eng, "tavb_search_messages_subset", eng.search_messages(q, K, np.float32(0.3), 4, subset_rows=SUBSET), q, 1, {3: 4, 4: K, 6: 4}, 5)
    np.testing.assert_array_equal(np.ctypeslib.as_array((ctypes.c_int64 * 4).from_address(_ptr(args[2]))), SUBSET)


def test_single_query_forms_refuse_a_wrong_shape_query():
    for call in (lambda e, q: e.search_subset(q, SUBSET, K, 0.3), lambda e, q: e.search_subset_topk(q, SUBSET, K, 0.3),
                 lambda e, q: e.search_subset_resident(q, _rows(), K, 0.3), lambda e, q: e.search_messages(q, K, 0.3, 4)):
        eng = _engine()
        with pytest.raises(ValueError, match=rf"not aligned: query must have {DIM} elements"):
            call(eng, np.zeros(DIM + 1, np.float32))
        assert eng.lib.calls == []


# ---- device-query and merge forms: what a host reaches are the refusals ---------------------------------------------------------------------

def _dq(dtype=torch.float32, nq=NQ):
    return torch.zeros((nq, DIM), dtype=dtype)


DEVICE_FORMS = [
    ("search_device", lambda e, dq, out: e.search_device(dq, K, 0.5, out_keys=out)),
    ("search_allgather", lambda e, dq, out: e.search_allgather(dq, K, 0.5, out_keys=out)),
    ("search_topk_device", lambda e, dq, out: e.search_topk_device(dq, K, 0.5, out_keys=out)),
    ("search_topk_allgather", lambda e, dq, out: e.search_topk_allgather(dq, K, 0.5, out_keys=out)),
    ("search_subset_batch_device", lambda e, dq, out: e.search_subset_batch_device(dq, _rows(), K, 0.5, out_keys=out)),
    ("search_masked_device", lambda e, dq, out: e.search_masked_device(dq, _bits(), K, 0.5, out_keys=out)),
    ("search_masked_wide_device", lambda e, dq, out: e.search_masked_wide_device(dq, _bits(), _rows(), K, 0.5, out_keys=out)),
]


@pytest.mark.parametrize("name,call", DEVICE_FORMS, ids=[n for n, _ in DEVICE_FORMS])
def test_device_forms_refuse_before_any_call(name, call):
    eng = _engine()
    with pytest.raises(AssertionError):
        call(eng, _dq(torch.float64), None)
    with pytest.raises(AssertionError):
        call(eng, torch.zeros((NQ, 2 * DIM))[:, :DIM], None)  # strided
    with pytest.raises(ValueError, match="out_keys must be an int64 torch tensor"):
        call(eng, _dq(), torch.zeros((NQ, K), dtype=torch.int32))
    with pytest.raises(ValueError, match=f"out_keys holds {2 * K} keys; this lookup writes {NQ} x {K} = {NQ * K}"):
        call(eng, _dq(), torch.zeros((2, K), dtype=torch.int64))
    with pytest.raises(ValueError, match="out_keys must live on cuda:0 or in pinned host memory"):
        call(eng, _dq(), torch.zeros((NQ, K), dtype=torch.int64))
    assert eng.lib.calls == []


def test_search_topk_device_counts_the_queries_of_a_flat_tensor():
    eng = _engine()
    with pytest.raises(ValueError, match=f"out_keys holds {K} keys; this lookup writes {NQ} x {K} = {NQ * K}"):
        eng.search_topk_device(torch.zeros(NQ * DIM), K, 0.5, out_keys=torch.zeros((1, K), dtype=torch.int64))
    with pytest.raises(AssertionError):
        eng.search_topk_device(torch.zeros(NQ * DIM + 1), K, 0.5)
    assert eng.lib.calls == []


def test_search_subset_device_refuses_before_any_call():
    eng = _engine()
    with pytest.raises(AssertionError):
        eng.search_subset_device(torch.zeros((2, DIM)), _rows(), K, 0.5)
    with pytest.raises(AssertionError):
        eng.search_subset_device(torch.zeros(DIM), _rows().to(torch.int64), K, 0.5)
    with pytest.raises(ValueError, match=f"out_keys holds 2 keys; this lookup writes 1 x {K} = {K}"):
        eng.search_subset_device(torch.zeros(DIM), _rows(), K, 0.5, out_keys=torch.zeros(2, dtype=torch.int64))
    assert eng.lib.calls == []


MERGE_FORMS = [
    ("merge_device", lambda e, out: e.merge_device(torch.zeros((2, NQ, K), dtype=torch.int64), out_keys=out)),
    ("allgather_merge", lambda e, out: e.allgather_merge(torch.zeros((NQ, K), dtype=torch.int64), out_keys=out)),
    ("merge_topk_device", lambda e, out: e.merge_topk_device(torch.zeros((2, NQ, K), dtype=torch.int64), out_keys=out)),
    ("merge_topk_device_query_major", lambda e, out: e.merge_topk_device(torch.zeros((NQ, 2, K), dtype=torch.int64), out_keys=out, query_major=True)),
    ("allgather_merge_topk", lambda e, out: e.allgather_merge_topk(torch.zeros((NQ, K), dtype=torch.int64), out_keys=out)),
]


@pytest.mark.parametrize("name,call", MERGE_FORMS, ids=[n for n, _ in MERGE_FORMS])
def test_merge_forms_refuse_before_any_call(name, call):
    eng = _engine()
    with pytest.raises(ValueError, match="out_keys must be an int64 torch tensor"):
        call(eng, np.zeros((NQ, K), np.int64))
    with pytest.raises(ValueError, match="out_keys must be contiguous"):
        call(eng, torch.zeros((NQ, 2 * K), dtype=torch.int64)[:, :K])
    with pytest.raises(ValueError, match=f"out_keys holds {K} keys; this lookup writes {NQ} x {K} = {NQ * K}"):
        call(eng, torch.zeros((1, K), dtype=torch.int64))
    with pytest.raises(ValueError, match="out_keys must live on cuda:0 or in pinned host memory"):
        call(eng, torch.zeros((NQ, K), dtype=torch.int64))
    assert eng.lib.calls == []


@pytest.mark.parametrize("call", [
    lambda e: e.merge_device(torch.zeros((2, NQ, K), dtype=torch.int32)),
    lambda e: e.merge_topk_device(torch.zeros((NQ, K), dtype=torch.int64)),
    lambda e: e.allgather_merge(torch.zeros((NQ, 2 * K), dtype=torch.int64)[:, :K]),
    lambda e: e.allgather_merge_topk(torch.zeros(K, dtype=torch.int64)),
])
def test_merge_forms_assert_on_their_lists(call):
    eng = _engine()
    with pytest.raises(AssertionError):
        call(eng)
    assert eng.lib.calls == []
