"""GPU suite: the contract of every C-ABI entry point that tavb_lookup_masked.hip, tavb_lookup_topk.hip, tavb_row_edits.hip and
tavb_mask_entry.hip define, driven through the library handle itself on a corpus of 70 rows x 64 columns (fp32 and fp16, ordinal_base 5, a
row -> message map of 9 messages).  Per entry point:

  1. error paths in the order of the checks: code and text of every bad argument, and with two bad arguments the earlier check's text;
     what nq == 0 gives (OK in most forms, an error in three device forms).  Argument checks only: nothing a kernel would dereference;
  2. the empty answer: host forms zero every count and leave the other outputs alone, device forms write nq * k zero keys;
  3. one non-empty call against the oracle (rows) or its numpy group-by (messages), and what the call leaves in the options
     "masked_route", "last_graph", "last_direct" and "last_topk_refine" -- literals recorded from the library before its host files were
     reorganised.  Before the call the context is primed: a masked tile batch (route 2) and then a single-query lookup that replays a
     captured graph (last_graph 1) or takes the one-launch path (last_direct != 0);
  4. host forms whose keys land in pinned memory up to 4096 keys and in device memory beyond: the same answers on both sides of it.
"""

from __future__ import annotations

import ctypes
import re
from ctypes import byref, c_int32, c_int64

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_batch_cases as sb
from tests import scoped_tile_cases as stc
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

ROWS, DIM, BASE, NMSG, NQ_MAX = 70, 64, 5, 9, 65
INVALID, NO_CORPUS, UNSUPPORTED = -1, -3, -4
GUARD = 0x5A5A5A5A5A5A5A5A
DTYPES = ["float32", "float16"]
_worlds: dict = {}


def _torch():
    import torch

    return torch


class Off:
    """a pointer `by` bytes into a valid allocation: misaligned, never dereferenced"""

    def __init__(self, base, by=1):
        self.base, self.by = base, by


def ptr(v):
    if v is None or isinstance(v, (int, float)):
        return v
    if isinstance(v, Off):
        return ptr(v.base) + v.by
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, (c_int32, c_int64, _native.MaskInfo)):
        return byref(v)
    if isinstance(v, ctypes.Array):
        return v
    return v.data_ptr()  # a torch tensor


class World:
    """one context over the tiny corpus, its masks, row lists and queries"""

    def __init__(self, dtype: str):
        torch = _torch()
        self.dtype, self.f16 = dtype, dtype == "float16"
        self.eng = _native.Engine(0)
        self.lib, self.h = self.eng.lib, self.eng._h
        v, _ = make_corpus(ROWS, DIM, 28_001)
        self.held = v.astype(np.float16).astype(np.float32) if self.f16 else v
        self.corpus = torch.from_numpy(v.astype(np.float16) if self.f16 else v).cuda()
        self.eng.set_corpus_tensor(self.corpus, ordinal_base=BASE)
        self.rm = (np.arange(ROWS) * 7 % NMSG).astype(np.int32)
        self.dev_rm = torch.from_numpy(self.rm).cuda()
        assert self.lib.tavb_set_row_messages(self.h, self.dev_rm.data_ptr(), ROWS, NMSG) == 0
        self.qs = make_queries(NQ_MAX, DIM, 28_002)
        self.dqs = torch.from_numpy(self.qs).cuda()
        rng = np.random.default_rng(28_003)
        self.masks = [rng.random(ROWS) < p for p in (0.5, 0.3, 0.8, 0.6, 0.4)]
        self.masks[0][0] = self.masks[2][ROWS - 1] = True
        self.dev_masks = [self.bits(m) for m in self.masks]
        self.no_rows = self.bits(np.zeros(ROWS, dtype=bool))
        self.rows0 = np.flatnonzero(self.masks[0]).astype(np.int32)
        self.dev_rows0 = torch.from_numpy(self.rows0).cuda()
        self.eng.set_option("graph_max_bytes", 1 << 20)
        torch.cuda.synchronize()

    def bits(self, mask):
        return _torch().from_numpy(_native.pack_mask_bits(mask).view(np.int32).copy()).cuda()

    def mask_of(self, q):
        return self.masks[q % len(self.masks)]

    def mask_ptrs(self, nq, dev=None, hole=None, off=None):
        vals = [(dev or self.dev_masks)[q % len(dev or self.dev_masks)].data_ptr() for q in range(nq)]
        if hole is not None:
            vals[hole] = None
        if off is not None:
            vals[off] += 1
        return (ctypes.c_void_p * max(nq, 1))(*vals)

    def span(self, nq):
        rows = np.flatnonzero(np.logical_or.reduce([self.mask_of(q) for q in range(nq)]))
        return int(rows[0]), int(rows[-1])

    def option(self, name):
        return self.eng.get_option(name)

    def prime(self, graph: bool):
        """route 2, then a single-query lookup: a graph replay (last_graph 1, last_direct 0) or the one-launch path (last_direct != 0)"""
        lib, a = self.lib, _native._addr
        o, s, c, t = np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.float32)
        q = np.ascontiguousarray(self.qs[:1])
        first, last = self.span(1)
        assert lib.tavb_search_masked_batch(self.h, a(q), 1, self.dev_masks[0].data_ptr(), ROWS, first, last, 1, a(t), a(o), a(s), a(c)) == 0
        self.eng.set_option("graph_max_bytes", (1 << 20) if graph else 0)
        for _ in range(4):
            assert lib.tavb_search_batch(self.h, a(q), 1, 3, a(t), a(o), a(s), a(c)) == 0
            if not graph or self.option("last_graph") == 1:
                break
        assert self.option("masked_route") == 2 and self.option("last_graph") == int(graph) and (graph or self.option("last_direct") != 0)


def world(dtype) -> World:
    if dtype not in _worlds:
        _worlds[dtype] = World(dtype)
    return _worlds[dtype]


class Call:
    """an entry point and its arguments behind the context, in declaration order"""

    def __init__(self, w: World, name: str, **args):
        self.w, self.name, self.args = w, name, args

    def __call__(self, **over):
        assert set(over) <= set(self.args), (self.name, over)
        a = {**self.args, **over}
        rc = getattr(self.w.lib, self.name)(self.w.h, *[ptr(v) for v in a.values()])
        return rc, (self.w.lib.tavb_last_error() or b"").decode()

    def __getitem__(self, key):
        return self.args[key]


# ---- the arguments of every entry point ------------------------------------------------------------------------------------------------

def host_out(nq, k, counts=np.int32):
    return dict(out=np.full(max(nq * k, 1), -7, dtype=np.int64), out_scores=np.full(max(nq * k, 1), -7.0, dtype=np.float32),
                out_counts=np.full(max(nq, 1), -7, dtype=counts))


def dev_out(nq, k):
    return dict(out_keys=_torch().full((nq * k + 1,), GUARD, dtype=_torch().int64, device="cuda"))


def thr(nq):
    return np.zeros(max(nq, 1), dtype=np.float32)


def build(w: World, name: str, nq: int, k: int, empty: bool = False) -> Call:
    """the good call of `name` for nq queries at depth k; empty: the form of it that has nothing to scan"""
    q, dq = np.ascontiguousarray(w.qs[:max(nq, 1)]), w.dqs
    first, last = (1, 0) if empty else w.span(max(nq, 1))
    f1, l1 = (1, 0) if empty else w.span(1)
    n0 = 0 if empty else len(w.rows0)
    masks = w.mask_ptrs(nq, dev=[w.no_rows] if empty else None)
    device = name.endswith("_device")
    src = dict(dev_queries=dq) if device else dict(queries=q)
    out = dev_out(nq, k) if device else host_out(nq, k)
    one = dict(dev_bits=w.dev_masks[0], rows=ROWS, first_row=f1, last_row=l1)
    many = dict(dev_masks=masks, rows=ROWS)
    spanned = dict(dev_masks=w.mask_ptrs(nq), rows=ROWS, first_row=first, last_row=last)
    base = name[len("tavb_search_"):].removesuffix("_device") if name.startswith("tavb_search_") else name
    if base == "subset_batch_resident" or name == "tavb_search_subset_batch_device":
        return Call(w, name, **src, nq=nq, dev_rows=w.dev_rows0, n_subset=n0, k=k, min_scores=thr(nq), remap=1, **out)
    if base in ("masked_batch", "masked"):
        return Call(w, name, **src, nq=nq, **one, k=k, min_scores=thr(nq), **out)
    if base == "masked_wide":
        one["last_row"] = w.span(1)[1] if empty else l1
        one["first_row"] = w.span(1)[0] if empty else f1
        return Call(w, name, **src, nq=nq, **one, dev_rows=w.dev_rows0, n_allowed=n0, k=k, min_scores=thr(nq), **out)
    if base == "messages_masked":
        return Call(w, name, **src, nq=nq, **one, dev_rows=w.dev_rows0, n_allowed=len(w.rows0), k=k, min_scores=thr(nq), max_messages=2, route=2, **out)
    if base in ("scoped_batch", "scoped", "scoped_topk", "top_messages_scoped"):
        return Call(w, name, **src, nq=nq, **many, k=k, min_scores=thr(nq), **out)
    if base == "messages_scoped":
        return Call(w, name, **src, nq=nq, **many, k=k, min_scores=thr(nq), max_messages=2, **out)
    if base in ("scoped_tile", "scoped_wide"):
        return Call(w, name, **src, nq=nq, **spanned, k=k, min_scores=thr(nq), **out)
    if base in ("messages_scoped_tile", "messages_scoped_wide"):
        return Call(w, name, **src, nq=nq, **spanned, k=k, min_scores=thr(nq), max_messages=2, **out)
    if base == "messages_batch":
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), accept_msgs=np.array([1, 3, 4, 8], dtype=np.int32), n_accept=4, max_messages=2, **out)
    if base == "topk" and not device:
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), **out)
    if base == "topk":
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), dev_rows=w.dev_rows0 if empty else None, n_subset=0, **out)
    if base == "subset_topk":
        return Call(w, name, query=q, rows_host=w.rows0.astype(np.int64), n_subset=n0, k=k, min_score=0.0, **host_out(1, k) | dict(out_counts=c_int32(-7)))
    if base == "sorted":
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), max_total=nq * k, **host_out(nq, k, np.int64), out_total=c_int64(-7))
    if base == "subset_sorted":
        return Call(w, name, query=q, rows_host=w.rows0.astype(np.int64), n_subset=n0, k=k, min_score=0.0, max_total=k,
                    **host_out(1, k) | dict(out_counts=c_int64(-7)))
    if base == "subset_batch_sorted":
        return Call(w, name, **src, nq=nq, dev_rows=w.dev_rows0, n_subset=n0, k=k, min_scores=thr(nq), max_total=nq * k, **host_out(nq, k, np.int64),
                    out_total=c_int64(-7))
    if base == "scoped_sorted":
        return Call(w, name, **src, nq=nq, **many, k=k, min_scores=thr(nq), max_total=nq * k, **host_out(nq, k, np.int64), out_total=c_int64(-7))
    if base == "top_messages":
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), dev_rows=w.dev_rows0, n_rows=n0, **out)
    if base == "top_messages_tile":
        return Call(w, name, **src, nq=nq, k=k, min_scores=thr(nq), **one, **out)
    raise KeyError(name)


ROW_LOOKUPS = ["tavb_search_subset_batch_resident", "tavb_search_subset_batch_device", "tavb_search_masked_batch", "tavb_search_masked_device",
               "tavb_search_masked_wide", "tavb_search_masked_wide_device", "tavb_search_scoped_batch", "tavb_search_scoped_device",
               "tavb_search_scoped_tile", "tavb_search_scoped_tile_device", "tavb_search_scoped_wide", "tavb_search_scoped_wide_device",
               "tavb_search_topk", "tavb_search_topk_device", "tavb_search_subset_topk", "tavb_search_sorted", "tavb_search_subset_sorted",
               "tavb_search_subset_batch_sorted", "tavb_search_scoped_topk", "tavb_search_scoped_topk_device", "tavb_search_scoped_sorted"]
MESSAGE_LOOKUPS = ["tavb_search_messages_masked", "tavb_search_messages_scoped", "tavb_search_messages_scoped_tile", "tavb_search_messages_scoped_wide",
                   "tavb_search_messages_batch", "tavb_search_top_messages", "tavb_search_top_messages_device", "tavb_search_top_messages_tile",
                   "tavb_search_top_messages_tile_device", "tavb_search_top_messages_scoped", "tavb_search_top_messages_scoped_device"]
LOOKUPS = ROW_LOOKUPS + MESSAGE_LOOKUPS
WIDE = {n for n in LOOKUPS if "wide" in n}  # fp16 corpora only
SINGLE = {"tavb_search_subset_topk", "tavb_search_subset_sorted"}  # one query
NO_EMPTY = {"tavb_search_messages_batch", "tavb_search_topk", "tavb_search_sorted"}  # nothing to scan only on an empty corpus


def allowed_rows(w: World, name: str, q: int, nq: int) -> np.ndarray:
    """the rows query q of the good call may return"""
    if "scoped" in name:
        return np.flatnonzero(w.mask_of(q))
    if name in ("tavb_search_topk", "tavb_search_topk_device", "tavb_search_sorted", "tavb_search_messages_batch"):
        return np.arange(ROWS)
    return w.rows0


# ---- 1. error paths ----------------------------------------------------------------------------------------------------------------------

K0 = (dict(k=0), INVALID, r"k must be >= 1 \(got 0\)")
K0_LARGE = (dict(k=0), INVALID, r"k must be 1 \.\. 16384 \(got 0\)")
K_SORTED = (dict(k=-1), INVALID, r"k must be >= 0 \(0 = every survivor\)")
NQ_NEG = (dict(nq=-1), INVALID, r"nq must be >= 0")
NQ_LOW = (dict(nq=0), INVALID, r"nq must be >= 1")
COVERS = (dict(rows=69), INVALID, r"the mask covers 69 rows, the corpus has 70")
SPAN = (dict(first_row=-1), INVALID, r"mask span \[-1, \d+\] outside the corpus")
SPAN_END = (dict(last_row=70), INVALID, r"mask span \[\d+, 70\] outside the corpus")
NULL_Q = (dict(queries=None), INVALID, r"null argument")
NULL_DQ = (dict(dev_queries=None), INVALID, r"null argument")
NULL_KEYS = (dict(out_keys=None), INVALID, r"null argument")
NULL_COUNTS = (dict(out_counts=None), INVALID, r"null argument")
NULL_MASKS = (dict(dev_masks=None), INVALID, r"null dev_masks")
FUSED = (dict(k=257), UNSUPPORTED, r"k=257 exceeds the fused-select limit 256")
MAX_MSG = (dict(max_messages=-1), INVALID, r"max_messages must be >= 0")
SUBSET_LEN = (dict(n_subset=-1), INVALID, r"bad subset length")
ROW_LIST_LEN = (dict(n_allowed=-1), INVALID, r"bad row list length")
SORTED_HEAD = [K_SORTED, (dict(max_total=-1), INVALID, r"max_total must be >= 0"), (dict(out_total=None), INVALID, r"null argument")]


def holed(w, nq=3):
    return (dict(dev_masks=w.mask_ptrs(nq, hole=1)), INVALID, r"the mask of query 1 is null")


def crooked(w, nq=3):
    return (dict(dev_masks=w.mask_ptrs(nq, off=0)), INVALID, r"the mask of query 0 must be 4-byte aligned")


def scoped_errors(w, k_max, head=K0):
    return [head, NQ_NEG, COVERS, (dict(k=k_max + 1), INVALID, rf"a scoped batch serves 1 <= k <= {k_max} \(got {k_max + 1}\)"), NULL_MASKS, holed(w), crooked(w)]


def lookup_errors(w: World, name: str):
    """the bad arguments of `name` in the order of its checks: (overrides, code, text)"""
    device = name.endswith("_device")
    null_in, null_out = (NULL_DQ, NULL_KEYS) if device else (NULL_Q, NULL_COUNTS)
    tile_k = (dict(k=65), UNSUPPORTED, r"the masked tile serves 1 <= k <= 64 and rows of a multiple of 64 bytes \(k = 65, \d+ bytes\): use the gather route")
    scoped_tile_k = (dict(k=65), UNSUPPORTED, r"the scoped tile serves 1 <= k <= 64 and rows of a multiple of 64 bytes \(k = 65, \d+ bytes\): use the row-list route")
    wide_k = (dict(k=257), UNSUPPORTED, r"the masked wide route serves fp16 corpora of up to 16384 halves per row and 1 <= k <= 256 \(k = 257\): use another masked route")
    scoped_wide_k = (dict(k=257), UNSUPPORTED, r"the scoped wide route serves fp16 corpora of up to 16384 halves per row and 1 <= k <= 256 \(k = 257\): use the row-list route")
    wide_args = [ROW_LIST_LEN, SPAN_END, (dict(dev_rows=None), INVALID, r"null dev_bits / dev_rows"),
                 (dict(dev_bits=Off(w.dev_masks[0])), INVALID, r"dev_bits must be 4-byte aligned")]
    top_args = [K0_LARGE, (dict(n_rows=-1), INVALID, r"bad row list length"), (dict(dev_rows=None), INVALID, r"null dev_rows")]
    top_tile = [K0_LARGE, NQ_NEG, (dict(dev_bits=Off(w.dev_masks[0])), INVALID, r"misaligned mask \(dev_bits must be 4-byte aligned\)"), COVERS, SPAN_END]
    table = {
        "tavb_search_subset_batch_resident": [K0_LARGE, NQ_NEG, SUBSET_LEN, (dict(remap=2), INVALID, r"remap must be 0 \(positions\) or 1 \(corpus ordinals\)"),
                                              NULL_Q, (dict(dev_rows=None), INVALID, r"null dev_rows")],
        "tavb_search_subset_batch_device": [K0_LARGE, NQ_LOW, SUBSET_LEN, (dict(remap=2), INVALID, r"remap must be 0 \(positions\) or 1 \(global ordinals\)"),
                                            NULL_KEYS, (dict(dev_rows=None), INVALID, r"null dev_rows")],
        "tavb_search_masked_batch": [K0, NQ_NEG, COVERS, SPAN, (dict(dev_bits=None), INVALID, r"null dev_bits"), tile_k, null_in],
        "tavb_search_masked_wide": [K0, NQ_NEG, COVERS] + wide_args + [wide_k, null_in],
        "tavb_search_messages_masked": [K0, FUSED, MAX_MSG, (dict(route=0), INVALID, r"route must be 1 \(row list\), 2 \(32/64-query tile\) or 3 \(wide filter tile\), got 0"),
                                        NQ_NEG, COVERS, SPAN, tile_k, NULL_Q],
        "tavb_search_scoped_batch": scoped_errors(w, 256) + [null_in],
        "tavb_search_messages_scoped": [K0, FUSED, MAX_MSG, NQ_NEG, COVERS, NULL_MASKS, holed(w), NULL_COUNTS],
        "tavb_search_scoped_tile": [K0, NQ_NEG, COVERS, SPAN, NULL_MASKS, holed(w), crooked(w), scoped_tile_k, null_in],
        "tavb_search_messages_scoped_tile": [K0, FUSED, MAX_MSG, COVERS, SPAN, NULL_MASKS, holed(w), scoped_tile_k, NULL_Q],
        "tavb_search_scoped_wide": [K0, NQ_NEG, COVERS, SPAN, NULL_MASKS, holed(w), crooked(w), scoped_wide_k, null_in],
        "tavb_search_messages_scoped_wide": [K0, FUSED, MAX_MSG, COVERS, SPAN, NULL_MASKS, holed(w), NULL_Q],
        "tavb_search_messages_batch": [K0, FUSED, MAX_MSG, NQ_NEG, (dict(n_accept=-2), INVALID, r"bad accept list"), NULL_Q],
        "tavb_search_topk": [K0_LARGE, (dict(k=16385), INVALID, r"k must be 1 \.\. 16384 \(got 16385\)"), NQ_NEG, NULL_Q],
        "tavb_search_subset_topk": [K0_LARGE, (dict(n_subset=-1), INVALID, r"n_subset must be >= 0"), (dict(query=None), INVALID, r"null argument"),
                                    (dict(rows_host=None), INVALID, r"null rows_host")],
        "tavb_search_topk_device": [K0_LARGE, NQ_LOW, NULL_KEYS, SUBSET_LEN, (dict(dev_rows=w.dev_rows0, nq=2), INVALID, r"a subset goes with exactly one query"),
                                    (dict(n_subset=3), INVALID, r"null dev_rows")],
        "tavb_search_sorted": SORTED_HEAD + [NQ_NEG, NULL_Q],
        "tavb_search_subset_sorted": [K_SORTED, (dict(max_total=-1), INVALID, r"max_total must be >= 0"), (dict(out_counts=None), INVALID, r"null argument"),
                                      (dict(n_subset=-1), INVALID, r"n_subset must be >= 0"), (dict(query=None), INVALID, r"null argument"),
                                      (dict(rows_host=None), INVALID, r"null rows_host")],
        "tavb_search_subset_batch_sorted": SORTED_HEAD + [NQ_NEG, SUBSET_LEN, NULL_Q, (dict(dev_rows=None), INVALID, r"null dev_rows")],
        "tavb_search_scoped_topk": scoped_errors(w, 16384) + [null_in],
        "tavb_search_scoped_sorted": SORTED_HEAD + [NQ_NEG, COVERS, NULL_MASKS, holed(w), crooked(w), NULL_Q],
        "tavb_search_top_messages": top_args + [NQ_NEG if not device else NQ_LOW, null_in],
        "tavb_search_top_messages_tile": top_tile + ([NQ_LOW] if device else []) + [null_in],
        "tavb_search_top_messages_scoped": [K0_LARGE, NQ_NEG, COVERS, NULL_MASKS, holed(w), crooked(w), null_in],
    }
    if not device:
        return table[name]
    twin = {"tavb_search_masked_device": "tavb_search_masked_batch", "tavb_search_scoped_device": "tavb_search_scoped_batch"}.get(name, name[: -len("_device")])
    return table.get(name) or [e for e in table[twin] if e is not NULL_Q and e is not NULL_COUNTS] + [null_in, null_out]


def check_errors(call: Call, errors):
    for i, (over, code, text) in enumerate(errors):
        rc, msg = call(**over)
        assert rc == code and re.search(text, msg), (call.name, over, rc, msg)
        for later, _, _ in errors[i + 1:]:  # an earlier check speaks first
            if set(later) & set(over):
                continue
            rc, msg = call(**over, **later)
            assert rc == code and re.search(text, msg), (call.name, over, later, rc, msg)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", LOOKUPS)
def test_lookup_errors_come_in_the_order_of_the_checks(name, dtype):
    w = world(dtype)
    call = build(w, name, 1 if name in SINGLE else 3, 2)
    errors = lookup_errors(w, name)
    if name in WIDE and not w.f16:  # the refusal of the shape is the last argument check: everything before it still speaks first
        errors = [e for e in errors if e[1] != UNSUPPORTED and e[0].keys() & {"k", "nq", "rows", "first_row", "last_row", "n_allowed", "dev_rows", "dev_bits", "dev_masks", "max_messages"}]
        rc, msg = call()
        assert rc == UNSUPPORTED and re.search(r"the (masked|scoped) wide route serves fp16 corpora", msg), (name, rc, msg)
    check_errors(call, errors)
    if "nq" in call.args:  # no query: OK before any pointer is looked at -- but for the device forms that refuse it
        refused = any(e is NQ_LOW for e in errors)
        nulls = {key: None for key in ("queries", "dev_queries", "min_scores", "out", "out_scores", "out_counts", "out_keys", "dev_masks") if key in call.args}
        rc, msg = call(nq=0, **nulls)
        if name in WIDE and not w.f16:
            assert rc == UNSUPPORTED
        elif refused:
            assert rc == INVALID and re.search(r"nq must be >= 1", msg), (name, rc, msg)
        else:
            assert rc == 0, (name, rc, msg)


def test_messages_masked_checks_its_route_arguments():
    w = world("float16")
    call = build(w, "tavb_search_messages_masked", 3, 2)
    check_errors(Call(w, call.name, **{**call.args, "route": 1}), [COVERS, ROW_LIST_LEN, (dict(dev_rows=None), INVALID, r"null dev_rows"), NULL_Q])
    check_errors(Call(w, call.name, **{**call.args, "route": 3}), [COVERS, ROW_LIST_LEN, SPAN_END, (dict(dev_rows=None), INVALID, r"null dev_bits / dev_rows"), NULL_Q])
    f32 = build(world("float32"), call.name, 3, 2)
    rc, msg = f32(route=3)
    assert rc == UNSUPPORTED and "the masked wide route serves" in msg


def test_message_lookups_need_the_map():
    torch = _torch()
    eng = _native.Engine(0)
    eng.set_corpus_tensor(torch.zeros((ROWS, DIM), dtype=torch.float32, device="cuda"))
    w = world("float32")
    for name in MESSAGE_LOOKUPS:
        if name in WIDE:
            continue
        call = build(w, name, 3, 2)
        rc = getattr(eng.lib, name)(eng._h, *[ptr(v) for v in call.args.values()])
        assert rc == NO_CORPUS and b"no row -> message map set" in eng.lib.tavb_last_error(), name
    eng.close()


# ---- 2. the empty answer -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,k", [(1, 2), (3, 1)])
@pytest.mark.parametrize("name", [n for n in LOOKUPS if n not in NO_EMPTY])
def test_the_empty_answer(name, nq, k, dtype):
    w = world(dtype)
    if (name in WIDE and not w.f16) or (name in SINGLE | {"tavb_search_topk_device"} and nq != 1):  # (a row list goes with one query there)
        return
    call = build(w, name, nq, k, empty=True)
    rc, msg = call(route=1, n_allowed=0) if name == "tavb_search_messages_masked" else call()
    assert rc == 0, (name, rc, msg)
    if "out_keys" in call.args:
        w.eng.synchronize()
        keys = call["out_keys"].cpu().numpy()
        assert (keys[:-1] == 0).all() and keys[-1] == GUARD, name
        return
    counts = call["out_counts"]
    assert (counts.value if name in SINGLE else counts.tolist()) == (0 if name in SINGLE else [0] * nq), name
    assert (call["out"] == -7).all() and (call["out_scores"] == -7.0).all(), name  # nothing wrote the other outputs
    if "out_total" in call.args:
        assert call["out_total"].value == 0


# ---- 3. one non-empty call per entry point, and what it leaves in the context -------------------------------------------------------------

def results(call: Call, nq: int, k: int):
    """per query (ordinals, scores) of the call that just ran"""
    if "out_keys" in call.args:
        call.w.eng.synchronize()
        keys = call["out_keys"].cpu().numpy()
        assert keys[-1] == GUARD, call.name
        o, s, c = _native.decode_keys(keys[:-1].view(np.uint64).reshape(nq, k))
        return [(o[i, : c[i]], s[i, : c[i]]) for i in range(nq)]
    counts = call["out_counts"]
    if call.name in SINGLE:
        return [(call["out"][: counts.value], call["out_scores"][: counts.value])]
    if counts.dtype == np.int64:  # the sorted forms: one list behind the other
        ends = np.concatenate([[0], np.cumsum(counts[:nq])])
        assert call["out_total"].value == ends[-1]
        return [(call["out"][ends[i]: ends[i + 1]], call["out_scores"][ends[i]: ends[i + 1]]) for i in range(nq)]
    o, s = call["out"].reshape(-1, k), call["out_scores"].reshape(-1, k)
    return [(o[i, : counts[i]], s[i, : counts[i]]) for i in range(nq)]


def check_rows(w: World, name: str, got, nq: int, k: int, base: int = BASE):
    for i, (o, s) in enumerate(got):
        flat = allowed_rows(w, name, i, nq)
        sub = w.held[flat]
        assert len(o) == min(k, len(flat)), (name, i)
        vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, w.qs[i])), o - base, s, k, 0.0, candidate_ordinals=flat, referee=vo.f64_referee(sub, w.qs[i]))


def check_messages(w: World, name: str, got, nq: int, k: int):
    """the group-by in numpy: the best score of every message -- among the k best rows and cut to max_messages = 2 for the re-ranked forms,
    among every allowed row and cut to k for the top-messages forms"""
    top = "top_messages" in name
    for i, (o, s) in enumerate(got):
        flat = allowed_rows(w, name, i, nq)
        sc = vo.cosine_to_score(np.dot(w.held[flat], w.qs[i]).astype(np.float32))
        order = np.argsort(-sc, kind="stable")
        if not top:
            order = order[:k]
        best: dict = {}
        for j in order:
            m = int(w.rm[flat[j]])
            if name == "tavb_search_messages_batch" and m not in (1, 3, 4, 8):
                continue
            best.setdefault(m, float(sc[j]))
        want = sorted(best.items(), key=lambda t: -t[1])[: k if top else 2]
        assert o.tolist() == [m for m, _ in want], (name, i, o, want)
        np.testing.assert_allclose(s, [x for _, x in want], atol=1e-5, rtol=0)


# (masked_route, last_graph after a graph replay, last_direct after a one-launch lookup, last_topk_refine) once the call is done
STATES = {
    "tavb_search_masked_batch": (2, 0, 0, 0),
    "tavb_search_masked_device": (2, 1, 0, 0),
    "tavb_search_masked_wide": (3, 0, 0, 0),
    "tavb_search_masked_wide_device": (3, 1, 0, 0),
    "tavb_search_messages_masked": (2, 0, 0, 0),
    "tavb_search_messages_masked:1": (1, 0, 0, 0),
    "tavb_search_messages_masked:3": (3, 0, 0, 0),
    "tavb_search_messages_scoped": (4, 0, 0, 0),
    "tavb_search_messages_scoped_tile": (5, 0, 0, 0),
    "tavb_search_messages_scoped_wide": (6, 0, 0, 0),
    "tavb_search_scoped_batch": (4, 0, 0, 0),
    "tavb_search_scoped_device": (4, 0, 0, 0),
    "tavb_search_scoped_sorted": (8, 0, 0, 0),
    "tavb_search_scoped_tile": (5, 0, 0, 0),
    "tavb_search_scoped_tile_device": (5, 1, 0, 0),
    "tavb_search_scoped_topk": (7, 0, 0, 0),
    "tavb_search_scoped_topk_device": (7, 0, 0, 0),
    "tavb_search_scoped_wide": (6, 0, 0, 0),
    "tavb_search_scoped_wide_device": (6, 0, 0, 0),
    "tavb_search_sorted": (2, 1, 1, 0),
    "tavb_search_subset_batch_device": (1, 1, 0, 0),
    "tavb_search_subset_batch_resident": (1, 1, 0, 0),
    "tavb_search_subset_batch_sorted": (1, 1, 0, 0),
    "tavb_search_subset_sorted": (2, 1, 1, 0),
    "tavb_search_subset_topk": (2, 1, 1, 0),
    "tavb_search_top_messages": (2, 0, 0, 0),
    "tavb_search_top_messages_device": (2, 0, 0, 0),
    "tavb_search_top_messages_scoped": (9, 0, 0, 0),
    "tavb_search_top_messages_scoped_device": (9, 0, 0, 0),
    "tavb_search_top_messages_tile": (10, 0, 0, 0),
    "tavb_search_top_messages_tile_device": (10, 0, 0, 0),
    "tavb_search_topk": (2, 1, 1, 0),
    "tavb_search_topk_device": (2, 1, 1, 0),
    "tavb_search_messages_batch": {1: (2, 0, 0, 0), 3: (2, 0, 4, 0)},  # by nq: one query stays on the streaming scan, three take the grouped one-launch form
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nq,k", [(1, 2), (3, 1), (3, 2)])
@pytest.mark.parametrize("name", LOOKUPS + ["tavb_search_messages_masked:1", "tavb_search_messages_masked:3"])
def test_one_call_and_what_it_leaves(name, nq, k, dtype):
    w = world(dtype)
    name, _, route = name.partition(":")
    if ((name in WIDE or route == "3") and not w.f16) or (name in SINGLE and nq != 1):
        return
    seen = []
    for graph in (True, False):
        w.prime(graph)
        call = build(w, name, nq, k)
        rc, msg = call(route=int(route)) if route else call()
        assert rc == 0, (name, rc, msg)
        got = results(call, nq, k)
        if name in SINGLE:  # positions in the row list
            got = [(w.rows0[o], s) for o, s in got]
        seen.append(tuple(w.option(o) for o in ("masked_route", "last_graph", "last_direct", "last_topk_refine")))
        base = 0 if name in SINGLE else BASE
        (check_rows(w, name, got, nq, k, base) if name in ROW_LOOKUPS else check_messages(w, name, got, nq, k))
    state = (seen[0][0], seen[0][1], seen[1][2], seen[0][3])
    assert seen[0][0] == seen[1][0] and seen[0][3] == seen[1][3]
    want = STATES[name + (":" + route if route else "")]
    assert state == (want[nq] if isinstance(want, dict) else want), (name, dtype, nq, k, state)


# ---- 4. on both sides of the pinned / device switch -------------------------------------------------------------------------------------

SWITCH = [("tavb_search_scoped_batch", 64, 64), ("tavb_search_scoped_tile", 64, 64), ("tavb_search_scoped_wide", 64, 64), ("tavb_search_masked_wide", 64, 64),
          ("tavb_search_subset_batch_resident", 4, 1024), ("tavb_search_scoped_topk", 4, 1024), ("tavb_search_top_messages", 4, 1024),
          ("tavb_search_top_messages_tile", 4, 1024), ("tavb_search_top_messages_scoped", 4, 1024)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,nq,k", SWITCH, ids=[s[0] for s in SWITCH])
def test_both_sides_of_the_pinned_key_limit(name, nq, k, dtype):
    w = world(dtype)
    if name in WIDE and not w.f16:
        return
    assert nq * k == 4096
    below, above = build(w, name, nq, k), build(w, name, nq + 1, k)
    for call in (below, above):
        rc, msg = call()
        assert rc == 0, (name, rc, msg)
    a, b = results(below, nq, k), results(above, nq + 1, k)
    for i in range(nq):
        assert a[i][0].tolist() == b[i][0].tolist() and a[i][1].view(np.uint32).tolist() == b[i][1].view(np.uint32).tolist(), (name, i)
    (check_rows if name in ROW_LOOKUPS else check_messages)(w, name, b, nq + 1, k)


# ---- the row edits -------------------------------------------------------------------------------------------------------------------------

def edit_world(dtype, capacity=ROWS):
    """a context of its own over a copy of the corpus: the edits write it"""
    torch = _torch()
    w = world(dtype)
    eng = _native.Engine(0)
    buf = torch.zeros((capacity, DIM), dtype=w.corpus.dtype, device="cuda")
    buf[:ROWS] = w.corpus
    eng.set_corpus_tensor(buf, rows=ROWS, ordinal_base=BASE)
    return w, eng, buf


def raw(eng, name, *args):
    rc = getattr(eng.lib, name)(eng._h, *[ptr(a) for a in args])
    return rc, (eng.lib.tavb_last_error() or b"").decode()


def check_raw(eng, name, good: dict, errors):
    for i, (over, code, text) in enumerate(errors):
        rc, msg = raw(eng, name, *{**good, **over}.values())
        assert rc == code and re.search(text, msg), (name, over, rc, msg)
        for later, _, _ in errors[i + 1:]:
            if not set(later) & set(over):
                rc, msg = raw(eng, name, *{**good, **over, **later}.values())
                assert rc == code and re.search(text, msg), (name, over, later, rc, msg)


def options(eng):
    return tuple(eng.get_option(o) for o in ("masked_route", "last_graph", "last_direct", "last_topk_refine"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_compact_rows(dtype):
    w, eng, buf = edit_world(dtype)
    remove = np.zeros(ROWS, dtype=bool)
    remove[[2, 3, 40, 69]] = True
    bits, nothing, out = w.bits(remove), w.bits(np.zeros(ROWS, dtype=bool)), c_int64(-7)
    good = dict(dev_remove_bits=bits, rows=ROWS, dev_dst=None, out_rows=out)
    check_raw(eng, "tavb_compact_rows", good, [
        (dict(out_rows=None), INVALID, r"null argument"), COVERS, (dict(dev_remove_bits=None), INVALID, r"null dev_remove_bits"),
        (dict(dev_remove_bits=Off(bits)), INVALID, r"dev_remove_bits must be 4-byte aligned"),
        (dict(dev_dst=Off(buf)), INVALID, r"the corpus and dev_dst must be aligned to their element size")])
    assert raw(eng, "tavb_compact_rows", nothing, ROWS, None, out)[0] == 0 and out.value == ROWS  # nothing to remove: no row moves
    eng.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), w.corpus.cpu().numpy())
    before = options(eng)
    rc, msg = raw(eng, "tavb_compact_rows", *good.values())
    assert rc == 0 and out.value == ROWS - 4, (rc, msg)
    eng.synchronize()
    np.testing.assert_array_equal(buf[: ROWS - 4].cpu().numpy(), np.delete(w.corpus.cpu().numpy(), np.flatnonzero(remove), axis=0))
    assert options(eng) == before
    other = _torch().zeros_like(buf)
    out2 = c_int64(-7)
    rc, msg = raw(eng, "tavb_compact_rows", w.bits(remove[: ROWS - 4]), ROWS - 4, other, out2)  # ... and into another buffer
    assert rc == 0 and out2.value == ROWS - 4 - int(remove[: ROWS - 4].sum()), (rc, msg)
    eng.synchronize()
    np.testing.assert_array_equal(other[: out2.value].cpu().numpy(), np.delete(buf[: ROWS - 4].cpu().numpy(), np.flatnonzero(remove[: ROWS - 4]), axis=0))
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_expand_rows(dtype):
    w, eng, buf = edit_world(dtype, capacity=ROWS + 8)
    new_rows = ROWS + 5
    holes = np.zeros(new_rows, dtype=bool)
    holes[[0, 7, 33, 34, 74]] = True
    bits, out = w.bits(holes), c_int64(-7)
    good = dict(dev_hole_bits=bits, new_rows=new_rows, dev_dst=None, out_old_rows=out)
    check_raw(eng, "tavb_expand_rows", good, [
        (dict(out_old_rows=None), INVALID, r"null argument"), (dict(new_rows=69), INVALID, r"the mask covers 69 rows, the corpus has 70 already"),
        (dict(new_rows=0x7FFFFFFF), UNSUPPORTED, r"at most 2\^31-2 rows per device shard \(got 2147483647\)"),
        (dict(dev_hole_bits=None), INVALID, r"null dev_hole_bits"), (dict(dev_hole_bits=Off(bits)), INVALID, r"dev_hole_bits must be 4-byte aligned"),
        (dict(dev_dst=Off(buf)), INVALID, r"the corpus and dev_dst must be aligned to their element size")])
    assert raw(eng, "tavb_expand_rows", w.bits(np.zeros(ROWS, dtype=bool)), ROWS, None, out)[0] == 0 and out.value == ROWS  # no hole: no row moves
    rc, msg = raw(eng, "tavb_expand_rows", bits, new_rows + 1, None, out)  # (one clear bit too many: found by the count pass, before any row moves)
    assert rc == INVALID and "the mask leaves 71 of 76 rows to the old rows, the corpus has 70" in msg, (rc, msg)
    eng.synchronize()
    np.testing.assert_array_equal(buf[:ROWS].cpu().numpy(), w.corpus.cpu().numpy())
    before = options(eng)
    rc, msg = raw(eng, "tavb_expand_rows", *good.values())
    assert rc == 0 and out.value == ROWS, (rc, msg)
    eng.synchronize()
    np.testing.assert_array_equal(buf[:new_rows].cpu().numpy()[~holes], w.corpus.cpu().numpy())
    assert options(eng) == before
    eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_scatter_rows(dtype):
    torch = _torch()
    w, eng, buf = edit_world(dtype)
    rows_host = np.ascontiguousarray(w.qs[:3])
    pos = torch.tensor([69, 0, 31], dtype=torch.int32, device="cuda")
    good = dict(rows_host=rows_host, n=3, dim=DIM, dev_positions=pos)
    check_raw(eng, "tavb_scatter_rows", good, [
        (dict(n=-1), INVALID, r"bad shape"), (dict(dim=63), INVALID, r"the rows are 63 wide, the corpus 64"), (dict(rows_host=None), INVALID, r"null pointer"),
        (dict(dev_positions=Off(pos)), INVALID, r"dev_positions must be 4-byte aligned"), (dict(n=71), INVALID, r"71 positions for 70 rows: they cannot be unique")])
    assert raw(eng, "tavb_scatter_rows", None, 0, DIM, None)[0] == 0  # no row: nothing to write
    bad = torch.tensor([69, 70, 31], dtype=torch.int32, device="cuda")
    rc, msg = raw(eng, "tavb_scatter_rows", rows_host, 3, DIM, bad)  # checked on the device before anything is written
    assert rc == INVALID and "a position is outside the corpus' 70 rows" in msg
    eng.synchronize()
    np.testing.assert_array_equal(buf.cpu().numpy(), w.corpus.cpu().numpy())
    before = options(eng)
    assert raw(eng, "tavb_scatter_rows", *good.values())[0] == 0
    want = w.corpus.cpu().numpy().copy()
    want[[69, 0, 31]] = rows_host.astype(want.dtype)
    np.testing.assert_array_equal(buf.cpu().numpy(), want)
    assert options(eng) == before
    eng.close()


# ---- the mask entry points -----------------------------------------------------------------------------------------------------------------

def unpack(words, rows):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:rows].astype(bool)


def test_mask_expand_and_pack():
    torch = _torch()
    w = world("float32")
    eng = w.eng
    rows_out, count = torch.full((ROWS + 1,), -7, dtype=torch.int32, device="cuda"), c_int64(-7)
    good = dict(dev_bits=w.dev_masks[0], rows=ROWS, dev_rows_out=rows_out, cap=ROWS, out_count=count)
    check_raw(eng, "tavb_mask_expand", good, [(dict(out_count=None), INVALID, r"null argument"), (dict(rows=-1), INVALID, r"rows must be 0 \.\. 2\^31 - 2"),
                                              (dict(cap=-1), INVALID, r"bad capacity"), (dict(dev_bits=None), INVALID, r"null dev_bits")])
    assert raw(eng, "tavb_mask_expand", None, 0, None, 0, count)[0] == 0 and count.value == 0
    before = options(eng)
    assert raw(eng, "tavb_mask_expand", *good.values())[0] == 0 and count.value == len(w.rows0)
    got = rows_out.cpu().numpy()
    assert got[: len(w.rows0)].tolist() == w.rows0.tolist() and (got[len(w.rows0):] == -7).all()
    rc, msg = raw(eng, "tavb_mask_expand", w.dev_masks[0], ROWS, rows_out, 3, count)
    assert rc == INVALID and re.search(rf"the mask has {len(w.rows0)} rows set, dev_rows_out holds 3", msg) and count.value == len(w.rows0)
    dev_bytes = torch.from_numpy(w.masks[1].astype(np.uint8) * 3).cuda()
    bits_out = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    good = dict(dev_bytes=dev_bytes, rows=ROWS, dev_bits_out=bits_out)
    check_raw(eng, "tavb_mask_pack", good, [(dict(rows=-1), INVALID, r"rows must be 0 \.\. 2\^31 - 2"), (dict(dev_bytes=None), INVALID, r"null argument")])
    assert raw(eng, "tavb_mask_pack", None, 0, None)[0] == 0
    assert raw(eng, "tavb_mask_pack", *good.values())[0] == 0
    eng.synchronize()
    words = bits_out.cpu().numpy()
    assert words[3] == -1 and words[:3].view(np.uint32).tolist() == _native.pack_mask_bits(w.masks[1]).tolist()
    assert options(eng) == before


def test_mask_from_messages_ranges_and_combine():
    torch = _torch()
    w = world("float16")
    eng = w.eng
    before = options(eng)
    accept = np.array([1, 3, 8, 42, -1], dtype=np.int32)
    bits_out = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    good = dict(accept=accept, n_accept=5, rows=ROWS, dev_bits_out=bits_out)
    check_raw(eng, "tavb_mask_from_messages", good, [COVERS, (dict(n_accept=-1), INVALID, r"bad accept list"), (dict(dev_bits_out=None), INVALID, r"null argument")])
    assert raw(eng, "tavb_mask_from_messages", *good.values())[0] == 0
    eng.synchronize()
    words = bits_out.cpu().numpy()
    assert words[3] == -1 and unpack(words[:3], ROWS).tolist() == np.isin(w.rm, [1, 3, 8]).tolist()
    # ranges: two collections over the rows, the row list and the info
    ranges = np.array([[3, 10], [40, 50], [5, 45]], dtype=np.int64)
    sizes = np.array([2, 1], dtype=np.int32)
    rows_out, info = torch.full((ROWS + 1,), -7, dtype=torch.int32, device="cuda"), _native.MaskInfo()
    good = dict(ranges=ranges, sizes=sizes, n_collections=2, domain=0, rows=ROWS, dev_bits_out=bits_out, dev_rows_out=rows_out, cap=ROWS, out_info=info)
    check_raw(eng, "tavb_mask_from_ranges", good, [
        (dict(out_info=None), INVALID, r"null argument"), (dict(domain=2), INVALID, r"domain must be 0 \(rows\) or 1 \(messages\), got 2"),
        (dict(n_collections=9), INVALID, r"a scope has 0 \.\. 8 collections \(got 9\)"), (dict(sizes=None), INVALID, r"null collection sizes"),
        (dict(ranges=None), INVALID, r"null ranges"), COVERS, (dict(cap=-1), INVALID, r"bad capacity"), (dict(dev_bits_out=None), INVALID, r"null dev_bits_out")])
    assert raw(eng, "tavb_mask_from_ranges", *good.values())[0] == 0
    want = np.flatnonzero(np.isin(np.arange(ROWS), list(range(5, 10)) + list(range(40, 45))))
    got = rows_out.cpu().numpy()
    assert (info.count, info.first_row, info.last_row) == (10, 5, 44) and got[:10].tolist() == want.tolist() and (got[10:] == -7).all()
    assert np.flatnonzero(unpack(bits_out.cpu().numpy()[:3], ROWS)).tolist() == want.tolist()
    rc, msg = raw(eng, "tavb_mask_from_ranges", *{**good, "cap": 4}.values())
    assert rc == INVALID and "the mask has 10 rows set, dev_rows_out holds 4" in msg
    assert raw(eng, "tavb_mask_from_ranges", *{**good, "n_collections": 1, "sizes": np.array([0], dtype=np.int32)}.values())[0] == 0
    assert (info.count, info.first_row, info.last_row) == (0, 0, -1)  # the empty mask
    # combine: masks[0] | masks[1], and-not
    ops = w.mask_ptrs(2)
    good = dict(op=_native.MASK_OR, dev_masks=ops, n_masks=2, rows=ROWS, dev_bits_out=bits_out, dev_rows_out=rows_out, cap=ROWS, out_info=info)
    check_raw(eng, "tavb_mask_combine", good, [
        (dict(out_info=None), INVALID, r"null argument"), (dict(op=3), INVALID, r"op must be 0 \(and\), 1 \(or\) or 2 \(and-not\), got 3"),
        (dict(n_masks=0), INVALID, r"a combination has 1 \.\. 8 operands \(got 0\)"), (dict(dev_masks=None), INVALID, r"null dev_masks"), COVERS,
        (dict(cap=-1), INVALID, r"bad capacity"), (dict(dev_bits_out=None), INVALID, r"null dev_bits_out"),
        (dict(dev_masks=w.mask_ptrs(2, hole=1)), INVALID, r"operand 1 is null")])
    for op, both in ((_native.MASK_OR, w.masks[0] | w.masks[1]), (_native.MASK_ANDNOT, w.masks[0] & ~w.masks[1])):
        rows_out.fill_(-7)
        assert raw(eng, "tavb_mask_combine", *{**good, "op": op}.values())[0] == 0
        want = np.flatnonzero(both)
        got = rows_out.cpu().numpy()
        assert (info.count, info.first_row, info.last_row) == (len(want), want[0], want[-1]) and got[: len(want)].tolist() == want.tolist() and (got[len(want):] == -7).all()
        assert unpack(bits_out.cpu().numpy()[:3], ROWS).tolist() == both.tolist()
    assert options(eng) == before


def test_mask_remap():
    torch = _torch()
    w = world("float32")
    eng = w.eng
    before = options(eng)
    remove = np.zeros(ROWS, dtype=bool)
    remove[[0, 2, 33, 64, 69]] = True
    flags, new_rows = w.bits(remove), ROWS - 5
    outs = [torch.full((4,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    lists = [torch.full((ROWS + 1,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
    arr = lambda ts: (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])  # noqa: E731
    info = (_native.MaskInfo * 2)()
    caps = np.array([ROWS, ROWS], dtype=np.int64)
    good = dict(mode=_native.REMAP_REMOVE, dev_flags=flags, old_rows=ROWS, new_rows=new_rows, dev_masks=w.mask_ptrs(2), dev_bits_out=arr(outs), n_masks=2, fill=0,
                dev_rows_out=arr(lists), caps=caps, out_info=info)
    check_raw(eng, "tavb_mask_remap", good, [
        (dict(n_masks=0), INVALID, r"a remap carries 1 \.\. 8 masks \(got 0\)"), (dict(out_info=None), INVALID, r"null argument"),
        (dict(mode=3), INVALID, r"mode must be 0 \(remove\), 1 \(insert\) or 2 \(append\), got 3"), (dict(old_rows=-1), INVALID, r"rows must be 0 \.\. 2\^31 - 2"),
        (dict(new_rows=71), INVALID, r"a removal from 70 rows cannot leave 71"), (dict(dev_flags=None), INVALID, r"null dev_flags"),
        (dict(dev_flags=Off(flags)), INVALID, r"dev_flags must be 4-byte aligned"), (dict(dev_bits_out=None), INVALID, r"null argument"),
        (dict(caps=None), INVALID, r"row lists without capacities"), (dict(dev_masks=w.mask_ptrs(2, hole=0)), INVALID, r"mask 0 is null")])
    rc, msg = raw(eng, "tavb_mask_remap", *{**good, "dev_bits_out": arr([outs[0], None])}.values())
    assert rc == INVALID and "output 1 is null" in msg
    rc, msg = raw(eng, "tavb_mask_remap", *{**good, "dev_masks": w.mask_ptrs(2, off=1)}.values())
    assert rc == INVALID and "mask 1 must be 4-byte aligned" in msg
    rc, msg = raw(eng, "tavb_mask_remap", *{**good, "dev_bits_out": arr([outs[0], w.dev_masks[0]])}.values())
    assert rc == INVALID and "output 1 overlaps mask or output 0" in msg
    rc, msg = raw(eng, "tavb_mask_remap", *{**good, "new_rows": new_rows - 1}.values())  # the count pass over the flags, before anything is written
    assert rc == INVALID and re.search(r"the flags have 65 clear bits among 70 rows, the edit needs 64", msg)
    eng.synchronize()
    assert all((t.cpu().numpy() == -1).all() for t in outs)
    assert raw(eng, "tavb_mask_remap", *good.values())[0] == 0
    for j in range(2):
        want = np.delete(w.masks[j], np.flatnonzero(remove))
        words, got = outs[j].cpu().numpy(), lists[j].cpu().numpy()
        rows = np.flatnonzero(want)
        assert words[3] == -1 and unpack(words[:3], new_rows).tolist() == want.tolist(), j
        assert (info[j].count, info[j].first_row, info[j].last_row) == (len(rows), rows[0], rows[-1]) and got[: len(rows)].tolist() == rows.tolist() and (got[len(rows):] == -7).all()
    rc, msg = raw(eng, "tavb_mask_remap", *{**good, "caps": np.array([ROWS, 2], dtype=np.int64)}.values())
    assert rc == INVALID and re.search(r"output 1 has \d+ rows set, its row list holds 2", msg)
    # an insertion: the same flags read as holes among 70 new rows
    back = [torch.full((4,), -1, dtype=torch.int32, device="cuda") for _ in range(2)]
    good.update(mode=_native.REMAP_INSERT, old_rows=new_rows, new_rows=ROWS, dev_masks=arr(outs), dev_bits_out=arr(back), fill=1)
    assert raw(eng, "tavb_mask_remap", *good.values())[0] == 0
    for j in range(2):
        assert unpack(back[j].cpu().numpy()[:3], ROWS).tolist() == (w.masks[j] | remove).tolist(), j
    assert options(eng) == before


def test_scope_planes_and_membership():
    torch = _torch()
    w = world("float16")
    eng = w.eng
    before = options(eng)
    n = 3
    first, last = w.span(n)
    blocks, words, _ = stc.plane_shape(n, first, last)
    planes = torch.full((blocks * words + 16,), -1, dtype=torch.int32, device="cuda")
    good = dict(dev_masks=w.mask_ptrs(n), n_masks=n, rows=ROWS, first_row=first, last_row=last, dev_planes_out=planes)
    check_raw(eng, "tavb_scope_planes", good, [
        (dict(n_masks=0), INVALID, r"n_masks must be >= 1"), (dict(rows=69), INVALID, r"the masks cover 69 rows, the corpus has 70"), SPAN_END,
        (dict(dev_masks=None), INVALID, r"null argument"), (dict(dev_planes_out=Off(planes, 4)), INVALID, r"dev_planes_out must be 64-byte aligned"),
        (dict(dev_masks=w.mask_ptrs(n, hole=1)), INVALID, r"mask 1 is null"), (dict(dev_masks=w.mask_ptrs(n, off=0)), INVALID, r"mask 0 must be 4-byte aligned")])
    assert raw(eng, "tavb_scope_planes", *{**good, "first_row": 1, "last_row": 0}.values())[0] == 0  # an empty span: no plane word to write
    eng.synchronize()
    assert (planes.cpu().numpy() == -1).all()
    assert raw(eng, "tavb_scope_planes", *good.values())[0] == 0
    eng.synchronize()
    got = planes.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got[: blocks * words].reshape(blocks, words), stc.planes_numpy([w.mask_of(q) for q in range(n)], first, last))
    assert (got[blocks * words:] == 0xFFFFFFFF).all()
    member = torch.full((len(w.rows0) + 8,), 0xAB, dtype=torch.uint8, device="cuda")
    good = dict(dev_masks=w.mask_ptrs(n), n_masks=n, rows=ROWS, dev_rows=w.dev_rows0, n=len(w.rows0), dev_member_out=member)
    check_raw(eng, "tavb_mask_membership", good, [
        (dict(n_masks=9), INVALID, r"a membership test has 1 \.\. 8 masks \(got 9\)"), (dict(rows=-1), INVALID, r"rows must be 0 \.\. 2\^31 - 2"),
        (dict(n=-1), INVALID, r"bad row list length"), (dict(dev_member_out=None), INVALID, r"null argument"),
        (dict(dev_rows=Off(w.dev_rows0)), INVALID, r"dev_rows must be 4-byte aligned"), (dict(dev_masks=w.mask_ptrs(n, hole=1)), INVALID, r"mask 1 is null"),
        (dict(dev_masks=w.mask_ptrs(n, off=2)), INVALID, r"mask 2 must be 4-byte aligned")])
    assert raw(eng, "tavb_mask_membership", *{**good, "n": 0, "dev_rows": None}.values())[0] == 0
    eng.synchronize()
    assert (member.cpu().numpy() == 0xAB).all()
    assert raw(eng, "tavb_mask_membership", *good.values())[0] == 0
    eng.synchronize()
    got = member.cpu().numpy()
    np.testing.assert_array_equal(got[: len(w.rows0)], sb.member_bytes([w.mask_of(q) for q in range(n)], w.rows0))
    assert (got[len(w.rows0):] == 0xAB).all()
    assert options(eng) == before


def test_sort_keys_device():
    torch = _torch()
    w = world("float32")
    eng = w.eng
    keys = np.random.default_rng(28_004).integers(1, 1 << 62, size=101, dtype=np.int64)
    dev = torch.from_numpy(keys.copy()).cuda()
    check_raw(eng, "tavb_sort_keys_device", dict(dev_keys=dev, n=100), [(dict(n=-1), INVALID, r"n must be 0 \.\. 2\^32 - 1"), (dict(dev_keys=None), INVALID, r"null dev_keys")])
    assert raw(eng, "tavb_sort_keys_device", None, 0)[0] == 0
    before = options(eng)
    assert raw(eng, "tavb_sort_keys_device", dev, 100)[0] == 0
    got = dev.cpu().numpy()
    assert got[:100].tolist() == np.sort(keys[:100])[::-1].tolist() and got[100] == keys[100]
    assert options(eng) == before
