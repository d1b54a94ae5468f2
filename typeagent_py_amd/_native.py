"""ctypes binding of libtavb.so (C ABI in include/tavb.h) plus the device-side
corpus holder.  PyTorch-ROCm is used only as the owner of device buffers and as
the source of the HIP stream / torch.distributed; every computation on the
lookup path is a hand-written gfx950 kernel reached through this binding.

There is deliberately no CPU fallback here: if libtavb.so is missing or no
MI355X is visible, lookups raise `RuntimeError`.
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, byref, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint64, c_void_p

import numpy as np

ABI_VERSION = 7  # include/tavb.h TAVB_ABI_VERSION this binding was written against
TAVB_F32 = 0
TAVB_F16 = 1
MAX_FUSED_K = 256
MAX_LARGE_K = 16384  # TAVB_MAX_LARGE_K: largest k of tavb_search_topk (exact top-k after one corpus pass)
MAX_STREAM_QUERIES = 8
MASK_ROWS_PER_WORKGROUP = 16384  # TAVB_MASK_ROWS_PER_WORKGROUP: rows of a mask one workgroup of tavb_mask_expand covers
# scope algebra (tavb_mask_from_ranges, tavb_mask_combine): TAVB_MAX_SCOPE_COLLECTIONS, TAVB_MAX_MASK_OPERANDS, TAVB_MASK_AND / _OR / _ANDNOT,
# TAVB_SCOPE_LDS_RANGES (most merged intervals of a scope the range kernel stages in LDS), the most ranges of one scope
MAX_SCOPE_COLLECTIONS = 8
MAX_MASK_OPERANDS = 8
MASK_AND, MASK_OR, MASK_ANDNOT = 0, 1, 2
REMAP_REMOVE, REMAP_INSERT, REMAP_APPEND = 0, 1, 2  # TAVB_REMAP_*: the edits tavb_mask_remap carries masks through
SCOPE_LDS_RANGES = 1024
MAX_SCOPE_RANGES = 1 << 20
SCOPE_DOMAINS = {"rows": 0, "messages": 1}

KERNEL_SCAN, KERNEL_MERGE, KERNEL_MFMA, KERNEL_NORMALIZE, KERNEL_CONVERT, KERNEL_MFMA_SAMPLE, KERNEL_SKINNY, KERNEL_RESCORE, KERNEL_EXCHANGE, KERNEL_TOPK = range(10)
COMM_ID_BYTES = 128

_LIB_NAME = os.environ.get("TAVB_LIBRARY", "libtavb.so")  # "libtavb_debug.so": the ASan/UBSan host build (`make -C csrc debug`)
_lib = None
_lib_lock = threading.Lock()

# (name, restype, argtypes) for every symbol declared in include/tavb.h
_SIGNATURES = [
    ("tavb_version", c_int, []),
    ("tavb_last_error", c_char_p, []),
    ("tavb_device_count", c_int, [POINTER(c_int)]),
    ("tavb_create", c_int, [c_int, c_void_p, POINTER(c_void_p)]),
    ("tavb_destroy", c_int, [c_void_p]),
    ("tavb_synchronize", c_int, [c_void_p]),
    ("tavb_set_option", c_int, [c_void_p, c_char_p, c_int64]),
    ("tavb_get_option", c_int, [c_void_p, c_char_p, POINTER(c_int64)]),
    ("tavb_set_corpus", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_int64]),
    ("tavb_upload_rows", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int32]),
    ("tavb_corpus_modified", c_int, [c_void_p, c_int64]),
    ("tavb_normalize_rows_f32", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32]),
    ("tavb_convert_f32_to_f16", c_int, [c_void_p, c_void_p, c_void_p, c_int64]),
    ("tavb_search", c_int, [c_void_p, c_void_p, c_int32, c_float, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_subset", c_int,
     [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_batch", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_set_row_messages", c_int, [c_void_p, c_void_p, c_int64, c_int64]),
    ("tavb_search_messages", c_int, [c_void_p, c_void_p, c_int32, c_float, c_void_p, c_int64, c_int32, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_messages_subset", c_int,
     [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_int32, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_begin", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    ("tavb_search_end", c_int, [c_void_p, c_int32, c_int32, c_void_p]),
    ("tavb_merge_keys_host", c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    ("tavb_merge_topk_host", c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    ("tavb_merge_top_messages_host", c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    ("tavb_search_all", c_int, [c_void_p, c_void_p, c_float, c_int64, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    ("tavb_search_subset_all", c_int,
     [c_void_p, c_void_p, c_void_p, c_int64, c_float, c_int64, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    ("tavb_search_topk", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_subset_topk", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_sorted", c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    ("tavb_search_subset_sorted", c_int,
     [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_float, c_int64, c_void_p, c_void_p, POINTER(c_int64)]),
    ("tavb_sort_keys_device", c_int, [c_void_p, c_void_p, c_int64]),
    ("tavb_search_after", c_int,
     [c_void_p, c_void_p, c_int32, c_float, c_float, c_int64, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_subset_after", c_int,
     [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_float, c_int64, c_void_p, c_void_p, POINTER(c_int32)]),
    ("tavb_search_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p]),
    ("tavb_search_topk_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_search_subset_device", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p]),
    ("tavb_search_subset_resident", c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int32, c_float, c_void_p, c_void_p, c_void_p]),
    ("tavb_mask_expand", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64, POINTER(c_int64)]),
    ("tavb_mask_pack", c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_search_subset_batch_resident", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_subset_batch_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p]),
    ("tavb_search_masked_batch", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_masked_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_masked_wide", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_masked_wide_device", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_mask_from_messages", c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    ("tavb_search_messages_masked", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_messages_batch", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_mask_from_ranges", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_mask_combine", c_int, [c_void_p, c_int32, c_void_p, c_int32, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_mask_remap", c_int, [c_void_p, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_batch", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_messages_scoped", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_mask_membership", c_int, [c_void_p, c_void_p, c_int32, c_int64, c_void_p, c_int64, c_void_p]),
    ("tavb_search_scoped_tile", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_tile_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_messages_scoped_tile", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_scope_planes", c_int, [c_void_p, c_void_p, c_int32, c_int64, c_int64, c_int64, c_void_p]),
    ("tavb_search_scoped_wide", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_wide_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_messages_scoped_wide", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_topk", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_scoped_topk_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_scoped_sorted", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    ("tavb_search_subset_batch_sorted", c_int,
     [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    ("tavb_search_top_messages", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_top_messages_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_search_top_messages_scoped", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_top_messages_scoped_device", c_int, [c_void_p, c_void_p, c_int32, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    ("tavb_search_top_messages_tile", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_top_messages_tile_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p]),
    ("tavb_plan_top_messages_tile", c_int, [c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int64, c_int64]),
    ("tavb_compact_rows", c_int, [c_void_p, c_void_p, c_int64, c_void_p, POINTER(c_int64)]),
    ("tavb_expand_rows", c_int, [c_void_p, c_void_p, c_int64, c_void_p, POINTER(c_int64)]),
    ("tavb_scatter_rows", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p]),
    ("tavb_merge_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    ("tavb_merge_topk_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p]),
    ("tavb_merge_top_messages_device", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p]),
    ("tavb_decode_keys", c_int, [c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_comm_unique_id", c_int, [c_void_p]),
    ("tavb_comm_init", c_int, [c_void_p, c_void_p, c_int32, c_int32]),
    ("tavb_comm_destroy", c_int, [c_void_p]),
    ("tavb_search_allgather", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p]),
    ("tavb_allgather_merge", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("tavb_search_topk_allgather", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    ("tavb_allgather_merge_topk", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("tavb_search_top_messages_allgather", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_allgather_merge_top_messages", c_int, [c_void_p, c_void_p, c_int32, c_int32, c_void_p]),
    ("tavb_remap_key_positions", c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int64]),
    ("tavb_search_rows", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_rows_device", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    ("tavb_search_rows_sorted", c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int64)]),
    ("tavb_gather_rows_f32", c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    ("tavb_join_pairs", c_int, [c_void_p, c_float, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    ("tavb_plan_pairs_join", c_int, [c_int64, c_int32, c_int32, c_int32, c_int32, c_int64]),
    ("tavb_profile_enable", c_int, [c_void_p, c_int32]),
    ("tavb_profile_reset", c_int, [c_void_p]),
    ("tavb_profile_read", c_int, [c_void_p, c_int32, POINTER(c_double), POINTER(c_int64)]),
    ("tavb_plan_ladder", c_int, [c_int64, c_int32, c_int32, POINTER(c_int64), c_int32]),
    ("tavb_plan_filter_shape", c_int, [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32]),
    ("tavb_plan_masked", c_int, [c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int64]),
    ("tavb_plan_masked_wide", c_int, [c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int64]),
    ("tavb_plan_scoped", c_int, [c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int64]),
    ("tavb_plan_scoped_wide", c_int, [c_int32, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_int64]),
]

ABI_SYMBOLS = [name for name, _, _ in _SIGNATURES]


_AS_POINTER = ctypes.c_char * 0  # `_AS_POINTER.from_buffer(ndarray)`: a ctypes object at the array's address, passed where a pointer is expected


def _addr(arr: np.ndarray):
    """The array's address as a ctypes argument: 0.25 us through the buffer protocol (writable arrays) against ~2 us for `ndarray.ctypes.data_as()`."""
    try:
        return _AS_POINTER.from_buffer(arr)
    except (TypeError, ValueError, BufferError):  # read-only (or otherwise not exportable) buffer
        return arr.ctypes.data_as(c_void_p)


def pack_mask_bits(mask: np.ndarray) -> np.ndarray:
    """bool [rows] -> the bit form tavb_mask_expand reads: uint32 [(rows + 31) // 32], row r = bit (r & 31) of word (r >> 5), the bits
    past `rows` zero.  Needs no GPU."""
    m = np.ascontiguousarray(mask)
    if m.dtype != np.bool_ or m.ndim != 1:
        raise TypeError("mask must be a 1-D bool array")
    packed = np.packbits(m, bitorder="little")
    words = np.zeros(((m.shape[0] + 31) // 32) * 4, dtype=np.uint8)
    words[: packed.shape[0]] = packed
    return words.view("<u4")


class MaskInfo(ctypes.Structure):
    """tavb_mask_info: a mask's count and span (an empty mask: 0, 0, -1)."""

    _fields_ = [("count", c_int64), ("first_row", c_int64), ("last_row", c_int64)]


def range_collections(collections) -> list[np.ndarray]:
    """The collections of a scope -- each a sequence of half-open integer (start, end) ranges, in any order, overlapping, duplicated or
    empty -- -> one int64 [m, 2] array each.  Needs no GPU."""
    out = []
    for c in collections:
        a = np.asarray(c if isinstance(c, np.ndarray) else list(c))
        if a.size == 0:
            a = np.zeros((0, 2), dtype=np.int64)
        if a.dtype.kind not in "iu":
            raise TypeError("range bounds must be integers")
        if a.ndim != 2 or a.shape[1] != 2:
            raise ValueError("a collection is a sequence of (start, end) pairs")
        out.append(np.ascontiguousarray(a, dtype=np.int64))
    if sum(len(a) for a in out) > MAX_SCOPE_RANGES:
        raise ValueError(f"a scope has at most {MAX_SCOPE_RANGES} ranges")
    return out


def merge_ranges(ranges: np.ndarray, n: int) -> np.ndarray:
    """int64 [m, 2] half-open ranges -> the same set inside [0, n) as disjoint ascending intervals, int64 [m', 2]: what
    tavb_mask_from_ranges does to every collection before the upload.  Needs no GPU."""
    a = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    s, e = np.maximum(a[:, 0], 0), np.minimum(a[:, 1], int(n))
    keep = s < e
    s, e = s[keep], e[keep]
    if s.size == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if int(n) >= 1 << 31:
        raise ValueError("ranges are merged over at most 2^31 - 1 values")
    key = np.sort((s << 32) | e)  # by start, then end: both fit 31 bits
    s, e = key >> 32, np.maximum.accumulate(key & 0xFFFFFFFF)
    opens = np.concatenate([[True], s[1:] > e[:-1]])  # an interval that starts beyond everything before it
    return np.stack([s[opens], e[np.concatenate([opens[1:], [True]])]], axis=1)


def ranges_to_bool(ranges: np.ndarray, n: int) -> np.ndarray:
    """bool [n]: the union of int64 [m, 2] half-open ranges inside [0, n).  Needs no GPU."""
    m = merge_ranges(ranges, n)
    edge = np.zeros(int(n) + 1, dtype=np.int64)
    np.add.at(edge, m[:, 0], 1)
    np.add.at(edge, m[:, 1], -1)
    return np.cumsum(edge[:-1]) > 0


def plan_ladder(rows: int, nq: int, n_cu: int = 256) -> list[int]:
    """Phase boundaries of the threshold ladder the library runs for a batch of `nq` (>= 65; >= 33 on corpora of 256 MiB and more) queries over `rows` rows with default options
    (tavb_plan_ladder): len(result) - 1 = tile-kernel launches per lookup.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    buf = (c_int64 * 16)()
    n = lib.tavb_plan_ladder(int(rows), int(nq), int(n_cu), buf, 16)
    _check(lib, n if n < 0 else 0)
    return [int(buf[i]) for i in range(n + 1)]


def plan_filter_shape(shape: int, query_tile: int = 256, split: bool = False, bdirect: bool = False, sched: int = 0, ablate: int = 0) -> int:
    """The MFMA shape (16 or 32) a filter launch of the 128/256-query tile runs on under these options (tavb_plan_filter_shape); raises on
    a shape or tile the engine refuses.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_filter_shape(int(shape), int(query_tile), int(bool(split)), int(bool(bdirect)), int(sched), int(ablate))
    _check(lib, r if r < 0 else 0)
    return int(r)


MASK_TILE_MIN_BYTES = 128 << 20  # the defaults of the options "mask_tile_min_bytes" / "mask_tile_pct"
MASK_TILE_PCT = 100


def plan_masked(nq: int, k: int, dim: int, dtype: int, allowed: int, span: int, min_bytes: int = MASK_TILE_MIN_BYTES, pct: int = MASK_TILE_PCT) -> bool:
    """True: a masked batch of `nq` queries with `allowed` set rows inside a span of `span` rows takes the 32/64-query tile under option
    "mask_tile" = 1, False: the gather route (tavb_plan_masked; dtype TAVB_F32 / TAVB_F16).  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_masked(int(nq), int(k), int(dim), int(dtype), int(allowed), int(span), int(min_bytes), int(pct))
    _check(lib, r if r < 0 else 0)
    return bool(r)


PAIRS_JOIN_MIN_ROWS = 8192  # the default of the option "pairs_join_min_rows" (provisional: tools/pairs_join_sweep.py has not run yet)
PAIRS_NO_FIT, PAIRS_REFUSED = 1, 2  # tavb_join_pairs' two answers that are no failures (include/tavb.h)


def plan_pairs_join(rows: int, dim: int, dtype: int, has_shadow: bool = True, single_gpu: bool = True, min_rows: int = PAIRS_JOIN_MIN_ROWS) -> bool:
    """True: `similarity_join` / `near_duplicate_pairs` of an index of `rows` x `dim` rows take the self-join under option "pairs_join" = 1,
    False: the row lookups (tavb_plan_pairs_join; dtype TAVB_F32 / TAVB_F16).  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_pairs_join(int(rows), int(dim), int(dtype), int(bool(has_shadow)), int(bool(single_gpu)), int(min_rows))
    _check(lib, r if r < 0 else 0)
    return bool(r)


TOP_MESSAGES_TILE_MIN_BATCH = 8  # the default of the option "top_messages_tile_min_batch"


def plan_top_messages_tile(nq: int, dim: int, dtype: int, allowed: int, span: int, min_batch: int = TOP_MESSAGES_TILE_MIN_BATCH,
                           min_bytes: int = MASK_TILE_MIN_BYTES, pct: int = MASK_TILE_PCT) -> bool:
    """True: a top-messages batch of `nq` queries with `allowed` allowed rows inside a span of `span` rows (both the corpus' rows for an
    unmasked lookup) takes the 32/64-query tile under option "top_messages_tile" = 1, False: the row scan of `search_top_messages`
    (tavb_plan_top_messages_tile; dtype TAVB_F32 / TAVB_F16).  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_top_messages_tile(int(nq), int(dim), int(dtype), int(allowed), int(span), int(min_batch), int(min_bytes), int(pct))
    _check(lib, r if r < 0 else 0)
    return bool(r)


MFMA_MIN_BATCH = 65  # the default of the option "mfma_min_batch": the fewest queries tavb_plan_masked_wide says yes to


def plan_masked_wide(nq: int, k: int, dim: int, dtype: int, allowed: int, span: int, min_bytes: int = MASK_TILE_MIN_BYTES, pct: int = MASK_TILE_PCT) -> bool:
    """True: a masked batch of `nq` queries with `allowed` set rows inside a span of `span` rows takes the 128/256-query filter tile +
    rescoring under option "mask_wide" = 1 (tavb_plan_masked_wide; fp16 corpora only).  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_masked_wide(int(nq), int(k), int(dim), int(dtype), int(allowed), int(span), int(min_bytes), int(pct))
    _check(lib, r if r < 0 else 0)
    return bool(r)


def plan_scoped(nq: int, k: int, dim: int, dtype: int, gather_rows: int, span: int, min_bytes: int = MASK_TILE_MIN_BYTES, pct: int = MASK_TILE_PCT) -> bool:
    """True: a scoped batch (one mask per query) of `nq` queries takes the 32/64-query tile under option "scope_tile" = 1, False: the
    row-list route (tavb_plan_scoped).  gather_rows: over the row-list route's passes of eight queries, the sum of each pass' largest
    scope (`scoped_gather_rows`); span: the rows of the span of the scopes' union.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_scoped(int(nq), int(k), int(dim), int(dtype), int(gather_rows), int(span), int(min_bytes), int(pct))
    _check(lib, r if r < 0 else 0)
    return bool(r)


def plan_scoped_wide(nq: int, k: int, dim: int, dtype: int, gather_rows: int, span: int, min_bytes: int = MASK_TILE_MIN_BYTES, pct: int = MASK_TILE_PCT) -> bool:
    """True: a scoped batch of `nq` queries takes the 128/256-query filter tile + rescoring under option "scope_wide" = 1
    (tavb_plan_scoped_wide); it then wins over `plan_scoped`.  gather_rows: `scoped_gather_rows` with passes of four queries for k > 64,
    eight otherwise; span: the rows of the span of the scopes' union.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    r = lib.tavb_plan_scoped_wide(int(nq), int(k), int(dim), int(dtype), int(gather_rows), int(span), int(min_bytes), int(pct))
    _check(lib, r if r < 0 else 0)
    return bool(r)


def scoped_gather_rows(counts, per_pass: int = 8) -> int:
    """`plan_scoped`'s gather_rows for scopes of `counts` rows in submission order: the largest scope of every pass of `per_pass` queries,
    summed -- a lower bound of the rows the row-list route reads (a pass reads the union of its scopes)."""
    counts = [int(c) for c in counts]
    return sum(max(counts[i : i + per_pass]) for i in range(0, len(counts), per_pass))


def scope_plane_shape(n_masks: int, first_row: int, last_row: int) -> tuple[int, int, int]:
    """(blocks of 32 queries, words per plane, first row of a plane) of tavb_scope_planes' output for that batch and span: the blocks of
    the tile-padded batch, rows first_row // 256 * 256 .. last_row rounded up to whole 32-row blocks."""
    begin = first_row // 256 * 256
    return (1 if n_masks <= 32 else 2 * ((n_masks + 63) // 64)), (last_row + 32) // 32 * 32 - begin, begin


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _LIB_NAME)


def load_library(preload_torch: bool = True):
    """dlopen libtavb.so and declare its prototypes.

    torch is imported first (when available) so that the process holds ONE HIP
    runtime: torch's bundled libamdhip64.so has the same SONAME
    (libamdhip64.so.7) as the ROCm one libtavb.so was linked against, so the
    dynamic loader reuses the copy that is already mapped.
    """
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not os.path.isfile(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C typeagent_py_amd/csrc`). There is no CPU fallback."
            )
        if preload_torch:
            try:
                import torch  # noqa: F401
            except Exception:  # pragma: no cover - torch is part of the image
                pass
        lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        try:
            lib.tavb_version.restype = c_int
            lib.tavb_version.argtypes = []
            found = int(lib.tavb_version())
        except AttributeError as exc:
            raise RuntimeError(f"{path} is not a libtavb build (no tavb_version): rebuild it with `make -C typeagent_py_amd/csrc`") from exc
        if found != ABI_VERSION:
            raise RuntimeError(f"{path} implements C ABI version {found}, this binding needs {ABI_VERSION} (include/tavb.h): "
                               "a stale build -- run `make -C typeagent_py_amd/csrc` (or check TAVB_LIBRARY)")
        for name, restype, argtypes in _SIGNATURES:
            fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
        return lib


class TavbError(RuntimeError):
    """A libtavb call failed (HIP/RCCL failures surface here, never as abort())."""


class TavbTimeout(TavbError):
    """`synchronize()`: an exchange of a collective lookup did not complete within the `comm_timeout_ms` option -- a peer never joined.  The
    library has aborted its communicator; `comm_init` again to rejoin."""


def _check(lib, rc: int) -> None:
    if rc != 0:
        msg = lib.tavb_last_error()
        text = msg.decode("utf-8", "replace") if msg else "unknown error"
        if rc == -1:
            raise ValueError(f"libtavb: {text}")
        if rc == -7:
            raise TavbTimeout(f"libtavb error {rc}: {text}")
        raise TavbError(f"libtavb error {rc}: {text}")


def device_count() -> int:
    lib = load_library()
    n = c_int(0)
    rc = lib.tavb_device_count(byref(n))
    if rc != 0:
        return 0
    return int(n.value)


def f32_threshold(min_score) -> np.float32:
    """The float32 `t` with (s >= t) == numpy's (s >= min_score) for float32 `s`.

    vectorbase.py:179 compares a float32 array with the caller's scalar.  Under
    NEP 50 a Python float/int is a weak scalar and is cast to float32 first
    (0.85 -> 0.8500000238...); a numpy float64 scalar forces a float64 compare,
    which equals comparing with the smallest float32 that is >= it.
    """
    if type(min_score) is float and -3.0e38 < min_score < 3.0e38:  # the common case, without the errstate context (1 us of a 30 us lookup)
        return np.float32(min_score)
    if isinstance(min_score, np.floating) and not isinstance(min_score, np.float32):
        wide = float(min_score)
        if wide != wide:
            return np.float32(np.nan)
        narrow = np.float32(wide)
        if float(narrow) < wide:
            narrow = np.nextafter(narrow, np.float32(np.inf), dtype=np.float32)
        return np.float32(narrow)
    with np.errstate(over="ignore"):
        return np.float32(min_score)


def batch_queries(queries, dim: int) -> np.ndarray:
    """A host batch of queries as the library reads it: contiguous float32 [nq, dim]."""
    a = np.ascontiguousarray(queries, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] != dim:
        raise ValueError(f"queries must be [nq, {dim}]")
    return a


def batch_thresholds(thrs, nq: int) -> np.ndarray:
    """float32 [nq] thresholds (or one for all) as the library reads them: contiguous float32 [nq].  The two shapes every caller in the
    package passes skip `np.broadcast_to`, whose read-only result also costs `_addr` its slow path: together 3 - 4 us of a batch's host time."""
    t = np.asarray(thrs, dtype=np.float32)
    if t.ndim == 0:
        return np.full(nq, t, dtype=np.float32)
    if t.shape == (nq,) and t.flags.c_contiguous:
        return t
    return np.ascontiguousarray(np.broadcast_to(t, (nq,)))


class Engine:
    """One libtavb context on one GPU + the torch tensors that hold the corpus."""

    def __init__(self, device: int | None = None, use_torch_stream: bool = False):
        import torch

        self._torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError(
                "typeagent_py_amd: no HIP device visible (torch.cuda.is_available() is False); "
                "the VectorBase engine runs on MI355X only and has no CPU fallback"
            )
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        stream_ptr = None
        if use_torch_stream:
            stream_ptr = c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        handle = c_void_p()
        _check(self.lib, self.lib.tavb_create(self.device, stream_ptr, byref(handle)))
        self._h = handle
        self._lock = threading.Lock()
        self._out_cache: dict = {}  # k -> reused output arrays of the single-query calls (+ their ctypes views)
        self.corpus = None  # torch tensor [capacity, dim]
        self._owns_corpus = False  # True when upload_rows allocated it (a tensor adopted from the caller is never appended into)
        self.rows = 0
        self.dim = 0
        self.dtype = TAVB_F32
        self.ordinal_base = 0
        # measurement / debugging hook: TAVB_ENGINE_OPTIONS="name=value,name=value" is applied to every context of the process (e.g. the GPU
        # suite under another kernel variant: TAVB_ENGINE_OPTIONS=mfma_sched=8 pytest -m gpu).  An unknown name raises, as set_option does.
        for item in filter(None, (x.strip() for x in os.environ.get("TAVB_ENGINE_OPTIONS", "").split(","))):
            name, _, val = item.partition("=")
            self.set_option(name.strip(), int(val))

    # -- lifecycle ---------------------------------------------------------
    def close(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h is not None and self.lib is not None:
            self.lib.tavb_destroy(h)
        self.corpus = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- options / profiling ----------------------------------------------
    def set_option(self, name: str, value: int) -> None:
        _check(self.lib, self.lib.tavb_set_option(self._h, name.encode(), int(value)))
        self.__dict__.pop("_mask_tile_opts", None)
        self.__dict__.pop("_mask_wide_opts", None)
        self.__dict__.pop("_scope_tile_opts", None)
        self.__dict__.pop("_scope_wide_opts", None)
        self.__dict__.pop("_top_messages_tile_opts", None)

    def top_messages_tile_options(self) -> tuple[int, int, int, int]:
        """("top_messages_tile", "top_messages_tile_min_batch", "mask_tile_min_bytes", "mask_tile_pct"), cached like `mask_tile_options`."""
        opts = self.__dict__.get("_top_messages_tile_opts")
        if opts is None:
            opts = self._top_messages_tile_opts = tuple(
                self.get_option(n) for n in ("top_messages_tile", "top_messages_tile_min_batch", "mask_tile_min_bytes", "mask_tile_pct"))
        return opts

    def mask_tile_options(self) -> tuple[int, int, int]:
        """("mask_tile", "mask_tile_min_bytes", "mask_tile_pct") as the library holds them, read once and again after any `set_option`: a
        masked batch asks on every call, and three option reads are 3 - 4 us of a 90 us lookup."""
        opts = self.__dict__.get("_mask_tile_opts")
        if opts is None:
            opts = self._mask_tile_opts = tuple(self.get_option(n) for n in ("mask_tile", "mask_tile_min_bytes", "mask_tile_pct"))
        return opts

    def mask_wide_options(self) -> tuple[int, int, int]:
        """("mask_wide", "mask_tile_min_bytes", "mask_tile_pct"), cached like `mask_tile_options`."""
        opts = self.__dict__.get("_mask_wide_opts")
        if opts is None:
            opts = self._mask_wide_opts = tuple(self.get_option(n) for n in ("mask_wide", "mask_tile_min_bytes", "mask_tile_pct"))
        return opts

    def scope_tile_options(self) -> tuple[int, int, int]:
        """("scope_tile", "mask_tile_min_bytes", "mask_tile_pct"), cached like `mask_tile_options`."""
        opts = self.__dict__.get("_scope_tile_opts")
        if opts is None:
            opts = self._scope_tile_opts = tuple(self.get_option(n) for n in ("scope_tile", "mask_tile_min_bytes", "mask_tile_pct"))
        return opts

    def scope_wide_options(self) -> tuple[int, int, int]:
        """("scope_wide", "mask_tile_min_bytes", "mask_tile_pct"), cached like `mask_tile_options`."""
        opts = self.__dict__.get("_scope_wide_opts")
        if opts is None:
            opts = self._scope_wide_opts = tuple(self.get_option(n) for n in ("scope_wide", "mask_tile_min_bytes", "mask_tile_pct"))
        return opts

    def get_option(self, name: str) -> int:
        out = c_int64(0)
        _check(self.lib, self.lib.tavb_get_option(self._h, name.encode(), byref(out)))
        return int(out.value)

    def profile_enable(self, on: bool = True) -> None:
        _check(self.lib, self.lib.tavb_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self) -> None:
        _check(self.lib, self.lib.tavb_profile_reset(self._h))

    def profile_read(self, kernel_id: int) -> tuple[float, int]:
        ms, n = c_double(0.0), c_int64(0)
        _check(self.lib, self.lib.tavb_profile_read(self._h, kernel_id, byref(ms), byref(n)))
        return float(ms.value), int(n.value)

    def synchronize(self) -> None:
        _check(self.lib, self.lib.tavb_synchronize(self._h))

    # -- corpus ------------------------------------------------------------
    def torch_dtype(self, dtype: int):
        return self._torch.float16 if dtype == TAVB_F16 else self._torch.float32

    def set_corpus_tensor(self, tensor, rows: int | None = None, ordinal_base: int = 0, sync_torch: bool = True, _owned: bool = False) -> None:
        """Adopt a device tensor [>=rows, dim] (f32 or f16, contiguous) as the corpus."""
        torch = self._torch
        if tensor.dim() != 2 or not tensor.is_contiguous():
            raise ValueError("corpus tensor must be a contiguous 2-D tensor")
        if tensor.device.type != "cuda" or (tensor.device.index or 0) != self.device:
            raise ValueError(f"corpus tensor must live on cuda:{self.device}")
        if tensor.dtype == torch.float32:
            dt = TAVB_F32
        elif tensor.dtype == torch.float16:
            dt = TAVB_F16
        else:
            raise ValueError("corpus tensor must be float32 or float16")
        n = tensor.shape[0] if rows is None else int(rows)
        if n > tensor.shape[0]:
            raise ValueError("rows exceeds the tensor")
        # make sure whatever produced the tensor on torch's stream has finished
        if sync_torch:
            torch.cuda.current_stream(self.device).synchronize()
        _check(self.lib, self.lib.tavb_set_corpus(self._h, c_void_p(tensor.data_ptr()), n, tensor.shape[1], dt, int(ordinal_base)))
        if not _owned and tensor is not self.corpus:
            # a caller's tensor: the allocator may have put it where a freed one of the same shape lived, and the library keys its
            # per-corpus caches (row-norm maxima, the fp16 shadow of an fp32 corpus) on the address
            _check(self.lib, self.lib.tavb_corpus_modified(self._h, 0))
        self.corpus, self.rows, self.dim, self.dtype, self.ordinal_base = tensor, n, int(tensor.shape[1]), dt, int(ordinal_base)
        self._owns_corpus = _owned

    def upload_rows(self, host_rows: np.ndarray, start: int, dtype: int, capacity_hint: int = 0) -> None:
        """Make device rows [start, start+len) equal to `host_rows` (f32), growing the
        buffer geometrically; rows [0, start) are kept (vectorbase.py:128/145 re-copies
        the whole matrix on every add; here an append moves only the new rows)."""
        torch = self._torch
        n_new = start + host_rows.shape[0]
        dim = host_rows.shape[1]
        tdt = self.torch_dtype(dtype)
        dev = torch.device("cuda", self.device)
        need_new = (
            self.corpus is None or self.corpus.shape[1] != dim or self.corpus.dtype != tdt or self.corpus.shape[0] < n_new
            or not self._owns_corpus  # adopted from the caller: copy into a buffer of our own before writing rows
        )
        if need_new:
            cap = max(n_new, capacity_hint, 2 * (self.corpus.shape[0] if self.corpus is not None and start > 0 else 0), 16)
            fresh = torch.empty((cap, dim), dtype=tdt, device=dev)
            if start > 0:
                if self.corpus is None or self.corpus.shape[1] != dim or self.corpus.dtype != tdt:
                    raise RuntimeError("cannot keep old rows across a layout change")
                fresh[:start].copy_(self.corpus[:start])
            self.corpus = fresh
        if host_rows.shape[0]:
            # pinned double-buffered staging + async H2D + on-device f32 -> f16 (tavb_upload_rows): no fp16 / second fp32 host copy
            src = np.ascontiguousarray(host_rows, dtype=np.float32)
            torch.cuda.current_stream(self.device).synchronize()  # the allocation / copy of old rows above ran on torch's stream
            dst = self.corpus.data_ptr() + start * dim * (2 if dtype == TAVB_F16 else 4)
            _check(self.lib, self.lib.tavb_upload_rows(self._h, _addr(src), src.shape[0], dim, c_void_p(dst), dtype))
        self.set_corpus_tensor(self.corpus, rows=n_new, ordinal_base=self.ordinal_base, _owned=True)
        _check(self.lib, self.lib.tavb_corpus_modified(self._h, int(start)))  # rows [start, n_new) were (re)written
        return True

    def mask_bits_to_device(self, words: np.ndarray):
        """A mask packed on the host (`pack_mask_bits`: uint32 words) -> torch int32 on this engine's device: rows / 8 bytes travel."""
        torch = self._torch
        return torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(torch.device("cuda", self.device))

    def compact_rows(self, dev_remove_bits) -> int:
        """Remove the rows whose bit is set in `dev_remove_bits` (torch int32 [(rows + 31) // 32] on this device, the layout of
        `pack_mask_bits`; set = remove) and move the others down in their old order (tavb_compact_rows): np.delete on the device ->
        the rows kept.  A corpus buffer this engine allocated is compacted in place; a tensor adopted from the caller is never written:
        its kept rows are gathered into a fresh tensor (capacity as `upload_rows` would pick), which becomes the owned corpus.  A mask
        with no bit set changes nothing."""
        torch = self._torch
        rows = self.rows
        if rows == 0 or self.corpus is None:
            return 0
        assert dev_remove_bits.dtype == torch.int32 and dev_remove_bits.is_contiguous() and dev_remove_bits.dim() == 1 and dev_remove_bits.numel() * 32 >= rows
        if dev_remove_bits.device.type != "cuda" or (dev_remove_bits.device.index or 0) != self.device:
            raise ValueError(f"the mask must live on cuda:{self.device}")
        fresh = None
        if not self._owns_corpus:
            fresh = torch.empty((max(rows, 16), self.dim), dtype=self.corpus.dtype, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()  # whatever produced the mask (and the allocation above) ran on torch's stream
        kept = c_int64(0)
        with self._lock:
            rc = self.lib.tavb_compact_rows(self._h, c_void_p(dev_remove_bits.data_ptr()), rows, c_void_p(fresh.data_ptr()) if fresh is not None else None,
                                            byref(kept))
        _check(self.lib, rc)
        self.synchronize()  # the moves were only enqueued: the mask, and an adopted tensor, may be released once they are done
        n = int(kept.value)
        if fresh is not None and n < rows:
            self.corpus, self._owns_corpus = fresh, True
        self.rows = n
        return n

    def _check_device_words(self, t, what: str) -> None:
        torch = self._torch
        assert t.dtype == torch.int32 and t.is_contiguous() and t.dim() == 1
        if t.device.type != "cuda" or (t.device.index or 0) != self.device:
            raise ValueError(f"{what} must live on cuda:{self.device}")

    def expand_rows(self, dev_hole_bits, new_rows: int) -> int:
        """Make room for new rows: `dev_hole_bits` (torch int32 [(new_rows + 31) // 32] on this device, the layout of `pack_mask_bits`)
        covers the NEW row count, a set bit is a hole; the old rows -- the clear bits must number `self.rows` -- move up in their old
        order to the rows whose bit is clear (tavb_expand_rows): the old rows of np.insert on the device -> how many old rows there
        were.  The holes hold anything until `scatter_rows` fills them.  A corpus buffer this engine allocated that holds `new_rows`
        rows is expanded in place; otherwise -- a tensor adopted from the caller, which is never written, or no capacity left -- the
        rows are placed in a fresh tensor of max(new_rows, twice the capacity, 16) rows, which becomes the owned corpus.  A mask with
        no bit set changes nothing."""
        torch = self._torch
        new_rows = int(new_rows)
        if self.corpus is None:
            raise RuntimeError("no corpus to expand: upload_rows() or set_corpus_tensor() first")
        self._check_device_words(dev_hole_bits, "the mask")
        assert dev_hole_bits.numel() * 32 >= new_rows
        fresh = None
        if new_rows > self.rows and (not self._owns_corpus or self.corpus.shape[0] < new_rows):
            fresh = torch.empty((max(new_rows, 2 * self.corpus.shape[0], 16), self.dim), dtype=self.corpus.dtype, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()  # whatever produced the mask (and the allocation above) ran on torch's stream
        old = c_int64(0)
        with self._lock:
            rc = self.lib.tavb_expand_rows(self._h, c_void_p(dev_hole_bits.data_ptr()), new_rows, c_void_p(fresh.data_ptr()) if fresh is not None else None,
                                           byref(old))
        _check(self.lib, rc)
        self.synchronize()  # the moves were only enqueued: the mask, and the old tensor, may be released once they are done
        if fresh is not None:
            self.corpus, self._owns_corpus = fresh, True
        self.rows = new_rows
        return int(old.value)

    def scatter_rows(self, host_rows: np.ndarray, positions) -> None:
        """Write `host_rows` (f32 [n, dim]) to corpus rows `positions` (n int32 ordinals, all different, each below `self.rows`: a torch
        int32 tensor on this device, or anything numpy makes one of -- 4 bytes a row travel), converted as `upload_rows` converts them
        (tavb_scatter_rows): the holes `expand_rows` left, or rows to overwrite.  The library's per-corpus caches survive: rows they cover
        get their fp16 shadow row written and their norms folded into the cached maxima.  A tensor adopted from the caller is never
        written: the corpus moves to a tensor of the engine's first."""
        torch = self._torch
        src = np.ascontiguousarray(host_rows, dtype=np.float32)
        if src.ndim != 2 or self.corpus is None or src.shape[1] != self.dim:
            raise ValueError(f"rows must be [n, {self.dim}]")
        if not isinstance(positions, torch.Tensor):
            positions = torch.from_numpy(np.ascontiguousarray(positions, dtype=np.int32).reshape(-1)).to(torch.device("cuda", self.device))
        self._check_device_words(positions, "the positions")
        if positions.numel() != src.shape[0]:
            raise ValueError(f"{positions.numel()} positions for {src.shape[0]} rows")
        if src.shape[0] == 0:
            return
        if not self._owns_corpus:
            self.set_corpus_tensor(self.corpus.clone(), rows=self.rows, ordinal_base=self.ordinal_base, _owned=True)
        torch.cuda.current_stream(self.device).synchronize()  # the positions (and the copy above) were made on torch's stream
        with self._lock:
            rc = self.lib.tavb_scatter_rows(self._h, _addr(src), src.shape[0], self.dim, c_void_p(positions.data_ptr()))
        _check(self.lib, rc)

    def clear(self) -> None:
        if self.corpus is not None:
            self.set_corpus_tensor(self.corpus, rows=0, ordinal_base=self.ordinal_base, _owned=self._owns_corpus)
        self.rows = 0

    # -- K1 / convert --------------------------------------------------------
    def normalize_rows_(self, tensor) -> None:
        torch = self._torch
        assert tensor.dtype == torch.float32 and tensor.is_contiguous() and tensor.dim() == 2
        torch.cuda.current_stream(self.device).synchronize()
        _check(self.lib, self.lib.tavb_normalize_rows_f32(self._h, c_void_p(tensor.data_ptr()), c_void_p(tensor.data_ptr()),
                                                          tensor.shape[0], tensor.shape[1]))
        self.synchronize()

    def normalize_rows(self, tensor):
        out = self._torch.empty_like(tensor)
        self._torch.cuda.current_stream(self.device).synchronize()
        _check(self.lib, self.lib.tavb_normalize_rows_f32(self._h, c_void_p(tensor.data_ptr()), c_void_p(out.data_ptr()),
                                                          tensor.shape[0], tensor.shape[1]))
        self.synchronize()
        return out

    def to_f16(self, tensor):
        torch = self._torch
        assert tensor.dtype == torch.float32 and tensor.is_contiguous()
        out = torch.empty(tensor.shape, dtype=torch.float16, device=tensor.device)
        torch.cuda.current_stream(self.device).synchronize()
        _check(self.lib, self.lib.tavb_convert_f32_to_f16(self._h, c_void_p(tensor.data_ptr()), c_void_p(out.data_ptr()), tensor.numel()))
        self.synchronize()
        return out

    # -- lookups -------------------------------------------------------------
    def _query(self, q) -> np.ndarray:
        a = np.ascontiguousarray(q, dtype=np.float32)
        if a.ndim != 1 or a.shape[0] != self.dim:
            raise ValueError(f"shapes ({self.rows},{self.dim}) and {tuple(np.shape(q))} not aligned: query must have {self.dim} elements")
        return a

    def _host_batch(self, queries, k: int, thrs):
        """The arguments and outputs of a host batch: (queries f32 [nq, dim], nq, thresholds f32 [nq], ordinals int64 [nq, k], scores f32
        [nq, k], counts int32 [nq], zeroed)."""
        a = batch_queries(queries, self.dim)
        nq = a.shape[0]
        return a, nq, batch_thresholds(thrs, nq), np.empty((nq, k), dtype=np.int64), np.empty((nq, k), dtype=np.float32), np.zeros(nq, dtype=np.int32)

    def _row_list(self, dev_rows):
        """A resident row list (torch int32 [S] on this device) -> (its address, S); an empty tensor has no address to name "a list" by: (None, 0)."""
        assert dev_rows.dtype == self._torch.int32 and dev_rows.is_contiguous() and dev_rows.dim() == 1
        n = int(dev_rows.numel())
        return (c_void_p(dev_rows.data_ptr()) if n else None), n

    def _single_query(self, k: int, call):
        """One query over a subset: `call(positions, scores, count)` -- the last three arguments of the library call -- fills k-sized
        outputs under the lock -> (positions int64[m], scores float32[m])."""
        pos = np.empty(k, dtype=np.int64)
        scs = np.empty(k, dtype=np.float32)
        cnt = c_int32(0)
        with self._lock:
            rc = call(_addr(pos), _addr(scs), byref(cnt))
        _check(self.lib, rc)
        m = int(cnt.value)
        return pos[:m], scs[:m]

    def _out_buffers(self, k: int):
        """Reused output arrays of the single-query calls, with their ctypes views: `ndarray.ctypes.data_as()` costs ~2 us a piece on the host --
        three of them were 6 us of a 33 us lookup on a 10k-row corpus.  Callers hold self._lock and copy the filled prefix out."""
        buf = self._out_cache.get(k)
        if buf is None:
            ords = np.empty(k, dtype=np.int64)
            scs = np.empty(k, dtype=np.float32)
            buf = self._out_cache[k] = (ords, scs, _AS_POINTER.from_buffer(ords), _AS_POINTER.from_buffer(scs), c_int32(0))
            if len(self._out_cache) > 16:
                self._out_cache.pop(next(iter(self._out_cache)))
        return buf

    def search(self, q, k: int, thr: np.float32, after: tuple[float, int] | None = None):
        """-> (ordinals int64[m], scores float32[m]) best first, m <= k <= MAX_FUSED_K."""
        a = self._query(q)
        try:
            pa = _AS_POINTER.from_buffer(a)  # 0.25 us; needs a writable buffer
        except (TypeError, ValueError):
            pa = _addr(a)
        with self._lock:
            ords, scs, p_ords, p_scs, cnt = self._out_buffers(k)
            if after is None:
                rc = self.lib.tavb_search(self._h, pa, k, c_float(float(thr)), p_ords, p_scs, byref(cnt))
            else:
                rc = self.lib.tavb_search_after(self._h, pa, k, c_float(float(thr)), c_float(after[0]), int(after[1]), p_ords, p_scs, byref(cnt))
            if rc == 0:
                m = int(cnt.value)
                out = ords[:m].copy(), scs[:m].copy()
        _check(self.lib, rc)
        return out

    def search_subset(self, q, rows: np.ndarray, k: int, thr: np.float32, after: tuple[float, int] | None = None):
        """rows: int64 corpus rows per subset position -> (positions int64[m], scores float32[m])."""
        a = self._query(q)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if after is None:
            return self._single_query(k, lambda *out: self.lib.tavb_search_subset(self._h, _addr(a), _addr(r), r.shape[0], k, c_float(float(thr)), *out))
        return self._single_query(k, lambda *out: self.lib.tavb_search_subset_after(self._h, _addr(a), _addr(r), r.shape[0], k, c_float(float(thr)),
                                                                                   c_float(after[0]), int(after[1]), *out))

    def rows_to_device(self, rows: np.ndarray):
        """int64 corpus rows (already wrapped and range-checked) -> torch int32 [S] on this engine's device."""
        torch = self._torch
        return torch.from_numpy(np.ascontiguousarray(rows, dtype=np.int32)).to(torch.device("cuda", self.device))

    def search_subset_resident(self, q, dev_rows, k: int, thr: np.float32):
        """`search_subset` over a row list that is already on the device (torch int32 [S], wrapped and range-checked by the caller)."""
        a = self._query(q)
        pos = np.empty(k, dtype=np.int64)
        scs = np.empty(k, dtype=np.float32)
        cnt = c_int32(0)
        # Written out, not `_single_query`: its closure and call are 1 us of this 7 us path (the repeated-subset lookup of a small index).
        # The address goes as it is, an empty list's included: `_row_list` would turn an empty view of a longer tensor into no pointer.
        with self._lock:
            rc = self.lib.tavb_search_subset_resident(self._h, _addr(a), c_void_p(dev_rows.data_ptr()), int(dev_rows.shape[0]), k,
                                                      c_float(float(thr)), _addr(pos), _addr(scs), byref(cnt))
        _check(self.lib, rc)
        m = int(cnt.value)
        return pos[:m], scs[:m]

    # row masks ---------------------------------------------------------------
    def expand_mask_bits(self, dev_bits, rows: int, cap: int | None = None):
        """Mask words on the device (torch int32 [(rows + 31) // 32], see `pack_mask_bits`) -> (torch int32 [count] on the device: the set
        rows below `rows` in ascending order, count) by tavb_mask_expand.  `cap`: the length of the output when the count is known (a
        smaller one raises ValueError); None asks the library for the count first -- a second call and synchronise, whose count pass reads
        the mask once more and whose write pass only sums the per-chunk counts."""
        torch = self._torch
        assert dev_bits.dtype == torch.int32 and dev_bits.is_contiguous() and dev_bits.numel() * 32 >= rows
        dev = torch.device("cuda", self.device)
        cnt = c_int64(0)
        with self._lock:
            if cap is None:
                rc = self.lib.tavb_mask_expand(self._h, c_void_p(dev_bits.data_ptr()), int(rows), None, 0, byref(cnt))
                _check(self.lib, rc)
                cap = int(cnt.value)
            out = torch.empty(max(int(cap), 0), dtype=torch.int32, device=dev)
            torch.cuda.current_stream(self.device).synchronize()
            rc = self.lib.tavb_mask_expand(self._h, c_void_p(dev_bits.data_ptr()), int(rows), c_void_p(out.data_ptr()) if cap else None, int(cap),
                                           byref(cnt))
        _check(self.lib, rc)
        n = int(cnt.value)
        return out[:n], n

    def pack_mask_tensor(self, mask, wait: bool = True):
        """A torch bool tensor [rows] on this engine's device -> its bit form on the device (torch int32 [(rows + 31) // 32], the layout of
        `pack_mask_bits`, tail bits zero) by tavb_mask_pack: rows / 8 bytes to expand here or -- after the synchronise of `wait` -- to copy out."""
        torch = self._torch
        if mask.dtype != torch.bool or mask.dim() != 1:
            raise TypeError("mask must be a 1-D bool tensor")
        if mask.device.type != "cuda" or (mask.device.index or 0) != self.device:
            raise ValueError(f"a tensor mask must live on cuda:{self.device}")
        rows = int(mask.shape[0])
        m = mask.contiguous()
        bits = torch.empty((rows + 31) // 32, dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()  # whatever produced the mask ran on torch's CURRENT stream (a caller inside another stream context waits for the producer itself)
        with self._lock:
            rc = self.lib.tavb_mask_pack(self._h, c_void_p(m.data_ptr()), rows, c_void_p(bits.data_ptr()))
        _check(self.lib, rc)
        if wait:
            self.synchronize()
        return bits

    def mask_to_rows(self, mask):
        """`mask_to_rows_bits` without the packed bits: (dev_rows, count)."""
        return self.mask_to_rows_bits(mask)[:2]

    def mask_to_rows_bits(self, mask):
        """An allow-mask -- a numpy bool array [rows], or a torch bool tensor [rows] on this engine's device -- -> (torch int32 [count] on
        the device: the allowed rows in ascending order, i.e. np.flatnonzero(mask); count).  A numpy mask is packed to bits on the host
        (rows / 8 bytes travel) and its count is known there; a device tensor is packed by tavb_mask_pack and never visits the host -- its
        count is not known, so the expansion is two calls (pack, count + sum, count + write: five launches, two synchronises).  Third: the packed mask on the device (torch int32 [(rows + 31) // 32]), what
        `search_masked_batch` reads."""
        torch = self._torch
        dev = torch.device("cuda", self.device)
        if isinstance(mask, torch.Tensor):
            bits = self.pack_mask_tensor(mask, wait=False)
            return (*self.expand_mask_bits(bits, int(mask.shape[0])), bits)  # (same stream: nothing to wait for)
        words = pack_mask_bits(np.asarray(mask))
        rows = int(np.shape(mask)[0])
        bits = torch.from_numpy(words.view(np.int32)).to(dev)
        torch.cuda.current_stream(self.device).synchronize()
        return (*self.expand_mask_bits(bits, rows, cap=int(np.count_nonzero(mask))), bits)

    # masked batches on the 32/64-query tile ------------------------------------------
    plan_masked = staticmethod(plan_masked)

    def _masked_args(self, dev_bits, span):
        torch = self._torch
        assert dev_bits.dtype == torch.int32 and dev_bits.is_contiguous() and dev_bits.dim() == 1 and dev_bits.numel() * 32 >= self.rows
        first, last = (0, self.rows - 1) if span is None else (int(span[0]), int(span[1]))
        return (c_void_p(dev_bits.data_ptr()) if dev_bits.numel() else None), first, last

    def search_masked_batch(self, queries, dev_bits, k: int, thrs, span=None):
        """A masked batch on the 32/64-query tile (tavb_search_masked_batch): queries f32 [nq, dim]; dev_bits torch int32 [(rows + 31) // 32]
        on this device, the mask over the whole corpus (`mask_to_rows_bits`, `pack_mask_tensor`); span = (first, last) allowed row (None:
        the whole corpus); 1 <= k <= 64; thrs float32 [nq] (or one for all) -> (ordinals [nq, k], scores [nq, k], counts [nq]), the layout
        of `search_batch`.  Raises TavbError (TAVB_E_UNSUPPORTED) for a shape the tile does not serve."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        bits, first, last = self._masked_args(dev_bits, span)
        with self._lock:
            rc = self.lib.tavb_search_masked_batch(self._h, _addr(a), nq, bits, int(self.rows), first, last, k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_masked_device(self, dev_queries, dev_bits, k: int, thrs, span=None, out_keys=None):
        """`search_masked_batch` with the queries on the device and nothing waited for (tavb_search_masked_device): dev_queries torch f32
        [nq, dim] -> torch int64 [nq, k] sorted, zero-padded keys carrying ordinal_base + row.  `out_keys`: a device tensor or a PINNED
        host tensor.  Async: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        bits, first, last = self._masked_args(dev_bits, span)
        with self._lock:
            rc = self.lib.tavb_search_masked_device(self._h, c_void_p(dev_queries.data_ptr()), nq, bits, int(self.rows), first, last, k, _addr(t),
                                                    c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    # masked batches on the 128/256-query filter tile + rescoring --------------------------
    plan_masked_wide = staticmethod(plan_masked_wide)

    def search_masked_wide(self, queries, dev_bits, dev_rows, k: int, thrs, span=None):
        """A masked batch on the 128/256-query filter tile with exact rescoring (tavb_search_masked_wide; fp16 corpora, 1 <= k <= 256): the
        arguments of `search_masked_batch` plus dev_rows, the mask's resident row list (torch int32 [count], ascending: `mask_to_rows_bits`),
        over which a query whose candidate band did not fit is re-run -> (ordinals [nq, k], scores [nq, k], counts [nq]), equal to
        `search_subset_batch_resident(queries, dev_rows, k, thrs)` bit for bit.  Raises TavbError (TAVB_E_UNSUPPORTED) for an fp32 corpus or a
        k the route does not serve."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        bits, first, last = self._masked_args(dev_bits, span)
        rows_ptr, n_allowed = self._row_list(dev_rows)
        with self._lock:
            rc = self.lib.tavb_search_masked_wide(self._h, _addr(a), nq, bits, int(self.rows), first, last, rows_ptr, n_allowed, k, _addr(t), _addr(ords),
                                                  _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_masked_wide_device(self, dev_queries, dev_bits, dev_rows, k: int, thrs, span=None, out_keys=None):
        """`search_masked_wide` with the queries on the device and the keys left there (tavb_search_masked_wide_device): torch int64 [nq, k]
        sorted, zero-padded keys carrying ordinal_base + row.  The call synchronises the stream once (the list of flagged queries is read
        back); `synchronize()` before reading the keys all the same."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        bits, first, last = self._masked_args(dev_bits, span)
        rows_ptr, n_allowed = self._row_list(dev_rows)
        with self._lock:
            rc = self.lib.tavb_search_masked_wide_device(self._h, c_void_p(dev_queries.data_ptr()), nq, bits, int(self.rows), first, last, rows_ptr, n_allowed, k,
                                                         _addr(t), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_subset_batch_resident(self, queries, dev_rows, k: int, thrs, remap: bool = True):
        """`search_subset_resident` for a batch: queries f32 [nq, dim] over ONE resident row list (torch int32 [S]: `mask_to_rows`, or
        wrapped, range-checked rows) in one submission, 1 <= k <= MAX_LARGE_K; thrs float32 [nq] (or one for all) -> (ordinals [nq, k],
        scores [nq, k], counts [nq]), the layout of `search_batch`.  remap=True: corpus ordinals (dev_rows ascending); False: positions."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        rows_ptr, n = self._row_list(dev_rows)
        with self._lock:
            rc = self.lib.tavb_search_subset_batch_resident(self._h, _addr(a), nq, rows_ptr, n, k, _addr(t),
                                                            1 if remap else 0, _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_all(self, q, thr: np.float32, max_out: int | None = None, subset_rows=None):
        """Every row (or subset position) with score >= thr, best first, in one corpus pass; the first `max_out` of them
        (None: all) -> (ordinals-or-positions int64[m], scores float32[m])."""
        a = self._query(q)
        r = None if subset_rows is None else np.ascontiguousarray(subset_rows, dtype=np.int64)
        cap = (self.rows if r is None else r.shape[0]) if max_out is None else min(int(max_out), self.rows if r is None else r.shape[0])
        items = np.empty(max(cap, 1), dtype=np.int64)
        scs = np.empty(max(cap, 1), dtype=np.float32)
        cnt, total = c_int64(0), c_int64(0)
        with self._lock:
            if r is None:
                rc = self.lib.tavb_search_all(self._h, _addr(a), c_float(float(thr)), cap, _addr(items),
                                              _addr(scs), byref(cnt), byref(total))
            else:
                rc = self.lib.tavb_search_subset_all(self._h, _addr(a), _addr(r), r.shape[0], c_float(float(thr)), cap,
                                                     _addr(items), _addr(scs), byref(cnt), byref(total))
        _check(self.lib, rc)
        m = int(cnt.value)
        return items[:m], scs[:m]

    def search_batch(self, queries, k: int, thrs):
        """queries f32 [nq, dim]; thrs float32 [nq] -> (ordinals [nq,k], scores [nq,k], counts [nq])."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        with self._lock:  # (five `ndarray.ctypes.data_as()` were 10 us of a 32 us two-query lookup on a small corpus)
            rc = self.lib.tavb_search_batch(self._h, _addr(a), nq, k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_topk(self, queries, k: int, thrs):
        """Exact top-k for any 1 <= k <= MAX_LARGE_K after one corpus pass per 8 queries (tavb_search_topk): queries f32 [nq, dim]; thrs
        float32 [nq] (or one for all) -> (ordinals [nq,k], scores [nq,k], counts [nq]), the layout of `search_batch`."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        with self._lock:
            rc = self.lib.tavb_search_topk(self._h, _addr(a), nq, k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_subset_topk(self, q, rows: np.ndarray, k: int, thr: np.float32):
        """`search_topk` of one query over a subset (rows: int64 corpus row per subset position) -> (positions int64[m], scores float32[m])."""
        a = self._query(q)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        return self._single_query(k, lambda *out: self.lib.tavb_search_subset_topk(self._h, _addr(a), _addr(r), r.shape[0], k, c_float(float(thr)), *out))

    def search_sorted(self, queries, k: int, thrs):
        """Every survivor (k = 0) or the best k for ANY k, sorted on the device after one corpus pass per 8 queries (tavb_search_sorted):
        queries f32 [nq, dim]; thrs float32 [nq] (or one for all) -> (ordinals int64 [total], scores float32 [total], counts int64 [nq]),
        query q's results at offsets counts[:q].sum() .. + counts[q].  Equal to `search_all` per query, bit for bit."""
        a = batch_queries(queries, self.dim)
        if k < 0:
            raise ValueError("k must be >= 0")
        nq = a.shape[0]
        t = batch_thresholds(thrs, nq)
        bound = nq * (self.rows if k == 0 else min(int(k), self.rows))
        ords = np.empty(max(bound, 1), dtype=np.int64)  # (lazy: only the pages the results touch are ever mapped)
        scs = np.empty(max(bound, 1), dtype=np.float32)
        cnts = np.zeros(nq, dtype=np.int64)
        total = c_int64(0)
        with self._lock:
            rc = self.lib.tavb_search_sorted(self._h, _addr(a), nq, int(k), _addr(t), bound, _addr(ords), _addr(scs), _addr(cnts), byref(total))
        _check(self.lib, rc)
        m = int(total.value)
        return ords[:m], scs[:m], cnts

    # -- rows of the corpus as queries ---------------------------------------
    def _positions(self, positions) -> np.ndarray:
        """Corpus rows (wrapped and range-checked by the caller) -> contiguous int32 [n]."""
        return np.ascontiguousarray(positions, dtype=np.int32).reshape(-1)

    def gather_rows(self, dev_positions, out=None):
        """Corpus rows dev_positions (torch int32 [n] on this device, each in [0, rows)) -> torch float32 [n, dim] on the device: the values the
        kernels multiply, fp16 rows widened exactly (tavb_gather_rows_f32).  Async: `synchronize()` before reading."""
        ptr, n = self._row_list(dev_positions)
        if out is None:
            out = self._torch.empty((n, self.dim), dtype=self._torch.float32, device=dev_positions.device)
        assert out.dtype == self._torch.float32 and out.is_contiguous() and out.numel() >= n * self.dim
        if n:
            with self._lock:
                rc = self.lib.tavb_gather_rows_f32(self._h, ptr, n, c_void_p(out.data_ptr()))
            _check(self.lib, rc)
        return out

    def search_rows(self, positions, k: int, thrs, exclude_self: bool = True):
        """The neighbours of corpus rows `positions` (int [n], each in [0, rows)) without the rows leaving the device (tavb_search_rows):
        thrs float32 [n] (or one for all); exclude_self: the row's own entry is taken out (1 <= k <= MAX_LARGE_K - 1), else the plain lookup
        with the rows as queries (k <= MAX_LARGE_K) -> (ordinals [n,k], scores [n,k], counts [n]), the layout of `search_batch`."""
        p = self._positions(positions)
        n = p.shape[0]
        t = batch_thresholds(thrs, n)
        ords, scs, cnts = np.empty((n, k), dtype=np.int64), np.empty((n, k), dtype=np.float32), np.zeros(n, dtype=np.int32)
        with self._lock:
            rc = self.lib.tavb_search_rows(self._h, _addr(p), n, k, 1 if exclude_self else 0, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def plans_pairs_join(self) -> bool:
        """Whether this engine's corpus takes the self-join: the switch "pairs_join" and tavb_plan_pairs_join under this engine's options."""
        return self.get_option("pairs_join") != 0 and plan_pairs_join(self.rows, self.dim, self.dtype, self.get_option("f32_shadow") != 0, True,
                                                                      self.get_option("pairs_join_min_rows"))

    def join_pairs(self, min_score, mask=None):
        """Every pair of corpus rows i < j scoring at least min_score (float32), both in `mask` where given (torch int32 packed mask on this
        device) -> (i int64 [m], j int64 [m], scores float32 [m]) in ARBITRARY order (tavb_join_pairs).  A call whose candidates do not fit
        "pairs_join_capacity" is made once more with the size it asked for, if that is within "pairs_join_max_capacity".  None: the join
        refused (a non-finite row: its bound proves nothing) or needs more than that -- the caller keeps the row lookups."""
        if mask is not None:
            self._check_device_words(mask, "the mask")
        cap = int(self.get_option("pairs_join_capacity"))
        for _ in range(2):
            out_i, out_j, out_s = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.float32)
            total, needed = c_int64(0), c_int64(0)
            with self._lock:
                rc = self.lib.tavb_join_pairs(self._h, c_float(float(min_score)), None if mask is None else c_void_p(mask.data_ptr()), cap, _addr(out_i),
                                              _addr(out_j), _addr(out_s), byref(total), byref(needed))
            if rc == PAIRS_REFUSED:
                return None
            if rc != PAIRS_NO_FIT:
                _check(self.lib, rc)
                m = int(total.value)
                return out_i[:m].copy(), out_j[:m].copy(), out_s[:m].copy()
            if needed.value <= cap or needed.value > self.get_option("pairs_join_max_capacity"):
                return None
            cap = int(needed.value)
        return None

    def search_rows_device(self, dev_positions, k: int, thrs, exclude_self: bool = True, out_keys=None, out_counts=None):
        """`search_rows` with the positions on the device (torch int32 [n]; the CALLER guarantees their range) and nothing waited for
        (tavb_search_rows_device) -> (torch int64 [n, k] sorted, zero-padded keys carrying global ordinals, torch int32 [n] counts).
        Async: `synchronize()` before reading."""
        torch = self._torch
        ptr, n = self._row_list(dev_positions)
        t = batch_thresholds(thrs, n)
        out_keys = self._out_keys(out_keys, n, k, dev_positions.device)
        if out_counts is None:
            out_counts = torch.empty(n, dtype=torch.int32, device=dev_positions.device)
        assert out_counts.dtype == torch.int32 and out_counts.is_contiguous() and out_counts.numel() >= n
        if n:
            with self._lock:
                rc = self.lib.tavb_search_rows_device(self._h, ptr, n, k, 1 if exclude_self else 0, _addr(t), c_void_p(out_keys.data_ptr()),
                                                      c_void_p(out_counts.data_ptr()))
            _check(self.lib, rc)
        return out_keys, out_counts

    def search_rows_sorted(self, positions, thrs, exclude_self: bool = True):
        """Every survivor per row (max_hits == 0), sorted on the device (tavb_search_rows_sorted) -> (ordinals int64 [total], scores float32
        [total], counts int64 [n]), the layout of `search_sorted`."""
        p = self._positions(positions)
        n = p.shape[0]
        t = batch_thresholds(thrs, n)
        bound = n * self.rows
        ords = np.empty(max(bound, 1), dtype=np.int64)
        scs = np.empty(max(bound, 1), dtype=np.float32)
        cnts = np.zeros(n, dtype=np.int64)
        total = c_int64(0)
        with self._lock:
            rc = self.lib.tavb_search_rows_sorted(self._h, _addr(p), n, 1 if exclude_self else 0, _addr(t), bound, _addr(ords), _addr(scs), _addr(cnts),
                                                  byref(total))
        _check(self.lib, rc)
        m = int(total.value)
        return ords[:m], scs[:m], cnts

    def search_subset_sorted(self, q, rows: np.ndarray, k: int, thr: np.float32):
        """`search_sorted` of one query over a subset (rows: int64 corpus row per subset position) -> (positions int64[m], scores float32[m])."""
        a = self._query(q)
        r = np.ascontiguousarray(rows, dtype=np.int64)
        if k < 0:
            raise ValueError("k must be >= 0")
        bound = r.shape[0] if k == 0 else min(int(k), r.shape[0])
        pos = np.empty(max(bound, 1), dtype=np.int64)
        scs = np.empty(max(bound, 1), dtype=np.float32)
        cnt = c_int64(0)
        with self._lock:
            rc = self.lib.tavb_search_subset_sorted(self._h, _addr(a), _addr(r), r.shape[0], int(k), c_float(float(thr)), bound, _addr(pos), _addr(scs),
                                                    byref(cnt))
        _check(self.lib, rc)
        m = int(cnt.value)
        return pos[:m], scs[:m]

    def sort_keys_device(self, dev_keys) -> None:
        """Sort a contiguous int64 device tensor of keys in place, descending as unsigned 64-bit values (tavb_sort_keys_device); synchronous."""
        torch = self._torch
        assert dev_keys.dtype == torch.int64 and dev_keys.is_contiguous() and dev_keys.dim() == 1
        with self._lock:
            rc = self.lib.tavb_sort_keys_device(self._h, c_void_p(dev_keys.data_ptr()), dev_keys.shape[0])
        _check(self.lib, rc)

    # message re-rank on the device ---------------------------------------------
    def set_row_messages(self, row_to_message: np.ndarray, n_messages: int | None = None) -> None:
        """int array [rows]: chunk row -> message ordinal (-1 = none); kept on the device next to the corpus.  n_messages: the number of
        messages when the rows are one shard of a larger corpus -- message ordinals are global, so every shard sets the same one (None:
        the map's largest ordinal + 1)."""
        torch = self._torch
        m = np.ascontiguousarray(row_to_message, dtype=np.int32)
        if m.ndim != 1:
            raise ValueError("row_to_message must be 1-D")
        self.row_messages = torch.from_numpy(m).to(torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()
        if n_messages is None:
            n_messages = int(m.max()) + 1 if m.size else 0
        self.n_messages = max(int(n_messages), 0)
        _check(self.lib, self.lib.tavb_set_row_messages(self._h, c_void_p(self.row_messages.data_ptr()), m.shape[0], max(n_messages, 0)))

    def search_messages(self, q, k: int, thr: np.float32, max_messages: int, accept=None, subset_rows=None):
        """-> (message ordinals int64[m], scores float32[m]).  accept: int array of accepted message ordinals (sqlite
        provider's subset form) or None; subset_rows: int64 corpus rows (memory provider's subset gather) or None."""
        a = self._query(q)
        if subset_rows is not None:
            r = np.ascontiguousarray(subset_rows, dtype=np.int64)
            return self._single_query(k, lambda *out: self.lib.tavb_search_messages_subset(self._h, _addr(a), _addr(r), r.shape[0], k, c_float(float(thr)),
                                                                                          int(max_messages), *out))
        acc = None if accept is None else np.ascontiguousarray(accept, dtype=np.int32)
        return self._single_query(k, lambda *out: self.lib.tavb_search_messages(self._h, _addr(a), k, c_float(float(thr)),
                                                                               _addr(acc) if acc is not None and acc.size else None,
                                                                               -1 if acc is None else acc.shape[0], int(max_messages), *out))

    # scoped and batched message lookups ------------------------------------------
    def mask_from_messages(self, accept):
        """A scope of MESSAGE ordinals (int array; ordinals outside the map's range are ignored, duplicates are harmless) -> (torch int32
        [count] on the device: the rows of those messages in ascending order; count; the packed mask, torch int32 [(rows + 31) // 32], tail
        bits zero) -- the triple of `mask_to_rows_bits`, built from the row -> message map on the device (tavb_mask_from_messages, then
        tavb_mask_expand): only the ordinals travel, no row list is made on the host.  Needs `set_row_messages`."""
        torch = self._torch
        acc = np.ascontiguousarray(accept, dtype=np.int32).reshape(-1)
        rows = int(self.rows)
        bits = torch.empty((rows + 31) // 32, dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()
        with self._lock:
            rc = self.lib.tavb_mask_from_messages(self._h, _addr(acc) if acc.size else None, int(acc.size), rows, c_void_p(bits.data_ptr()) if rows else None)
        _check(self.lib, rc)
        return (*self.expand_mask_bits(bits, rows), bits)  # (same stream: nothing to wait for)

    # scope algebra -------------------------------------------------------------------
    def _mask_algebra(self, call, bits, bound: int):
        """One tavb_mask_from_ranges / tavb_mask_combine call that writes `bits` and a row list of at most `bound` rows ->
        (dev_rows, count, bits, span), span = (first, last) set row or None.  A list that fills less than half of its bound is copied into
        a tensor of its own size, so that a small result does not pin a large allocation."""
        torch = self._torch
        bound = int(bound)
        out = torch.empty(bound, dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()
        info = MaskInfo()
        with self._lock:
            rc = call(c_void_p(out.data_ptr()) if bound else None, bound, byref(info))
        _check(self.lib, rc)
        n = int(info.count)
        dev_rows = out[:n].clone() if bound > 2 * n else out[:n]
        return dev_rows, n, bits, ((int(info.first_row), int(info.last_row)) if n else None)

    def mask_from_ranges(self, collections, domain="rows"):
        """The mask of a scope of ranges (tavb_mask_from_ranges): `collections`, up to 8 of them, each a sequence of half-open (start, end)
        ranges over the rows (domain "rows") or over the message ordinals of `set_row_messages` (domain "messages"); a row is set when
        every collection has a range that holds it (its message) -> (torch int32 [count] on the device: the set rows in ascending order;
        count; the packed mask, torch int32 [(rows + 31) // 32], tail bits zero; span = (first, last) set row, or None).  Rows: the
        merged ranges bound the count, so it is one call of two launches.  Messages: the mask and its count first (one launch), then
        the row list from the mask."""
        torch = self._torch
        dom = SCOPE_DOMAINS[domain] if isinstance(domain, str) else int(domain)
        cols = range_collections(collections)
        if len(cols) > MAX_SCOPE_COLLECTIONS:
            raise ValueError(f"a scope has at most {MAX_SCOPE_COLLECTIONS} collections (got {len(cols)})")
        rows = int(self.rows)
        ranges = np.ascontiguousarray(np.concatenate(cols)) if cols else np.zeros((0, 2), dtype=np.int64)
        sizes = np.array([len(c) for c in cols], dtype=np.int32)
        bits = torch.empty((rows + 31) // 32, dtype=torch.int32, device=torch.device("cuda", self.device))
        bits_ptr = c_void_p(bits.data_ptr()) if rows else None

        def call(out_ptr, cap, info):
            return self.lib.tavb_mask_from_ranges(self._h, _addr(ranges) if ranges.size else None, _addr(sizes) if sizes.size else None, len(cols), dom, rows,
                                                  bits_ptr, out_ptr, cap, info)

        if dom == 0:  # every collection's merged length bounds the count of their intersection
            bound = min((int(np.diff(merge_ranges(c, rows), axis=1).sum()) for c in cols), default=rows)
            return self._mask_algebra(call, bits, bound)
        _, n, _, span = self._mask_algebra(call, bits, 0)
        dev_rows, n = self.expand_mask_bits(bits, rows, cap=n)
        return dev_rows, n, bits, span

    def mask_combine(self, op: int, dev_bits_list, cap: int):
        """AND / OR / ANDNOT of 1 .. 8 packed masks on the device (tavb_mask_combine; op: MASK_AND, MASK_OR, MASK_ANDNOT = the first
        without the others, with one operand its complement) -> the quadruple of `mask_from_ranges`.  `cap`: a bound of the result's
        count (a smaller one raises ValueError); 0 asks for the mask, its count and its span only."""
        torch = self._torch
        masks = list(dev_bits_list)
        if not 1 <= len(masks) <= MAX_MASK_OPERANDS:
            raise ValueError(f"a combination has 1 .. {MAX_MASK_OPERANDS} operands (got {len(masks)})")
        rows = int(self.rows)
        for m in masks:
            assert m.dtype == torch.int32 and m.is_contiguous() and m.dim() == 1 and m.numel() * 32 >= rows
        ptrs = (c_void_p * len(masks))(*[m.data_ptr() for m in masks])
        bits = torch.empty((rows + 31) // 32, dtype=torch.int32, device=torch.device("cuda", self.device))
        bits_ptr = c_void_p(bits.data_ptr()) if rows else None
        return self._mask_algebra(lambda out_ptr, n, info: self.lib.tavb_mask_combine(self._h, int(op), ptrs, len(masks), rows, bits_ptr, out_ptr, n, info),
                                  bits, cap)

    def mask_remap(self, mode: int, dev_flags, old_rows: int, new_rows: int, dev_bits_list, fill, counts=None):
        """1 .. 8 packed masks carried through one row edit on the device (tavb_mask_remap) -> per mask the quadruple of `mask_combine`:
        (dev_rows, count, dev_bits, span) over `new_rows` rows, in fresh tensors.  mode REMAP_REMOVE: `dev_flags` (torch int32 on this
        device, the layout of `pack_mask_bits`) covers `old_rows`, a set bit removes the row -- np.delete of every mask; `new_rows` must be
        the number of clear bits.  REMAP_INSERT: `dev_flags` covers `new_rows`, a set bit is a hole that takes `fill` -- np.insert; the
        clear bits must number `old_rows`.  REMAP_APPEND: `dev_flags` is None, rows [old_rows, new_rows) take `fill`.  A mismatch raises
        ValueError before anything is written.  Bits of the inputs at or beyond `old_rows` are ignored.  `counts`: the inputs' counts
        when the caller knows them -- they bound the row lists; without them every list is allocated at `new_rows` first."""
        torch = self._torch
        masks = list(dev_bits_list)
        mode, old_rows, new_rows, fill = int(mode), int(old_rows), int(new_rows), bool(fill)
        if mode not in (REMAP_REMOVE, REMAP_INSERT, REMAP_APPEND):
            raise ValueError(f"mode must be REMAP_REMOVE, REMAP_INSERT or REMAP_APPEND, got {mode}")
        if not 1 <= len(masks) <= MAX_MASK_OPERANDS:
            raise ValueError(f"a remap carries 1 .. {MAX_MASK_OPERANDS} masks (got {len(masks)})")
        if old_rows < 0 or new_rows < 0 or (new_rows > old_rows if mode == REMAP_REMOVE else new_rows < old_rows):
            raise ValueError(f"an edit of mode {mode} cannot take {old_rows} rows to {new_rows}")
        if counts is not None and len(counts) != len(masks):
            raise ValueError(f"{len(counts)} counts for {len(masks)} masks")
        flag_rows = old_rows if mode == REMAP_REMOVE else new_rows if mode == REMAP_INSERT else 0
        if flag_rows:
            self._check_device_words(dev_flags, "the flags")
            if dev_flags.numel() * 32 < flag_rows:
                raise ValueError(f"the flags hold {dev_flags.numel()} words, {flag_rows} rows need {(flag_rows + 31) // 32}")
        for i, m in enumerate(masks):
            self._check_device_words(m, f"mask {i}")
            if m.numel() * 32 < old_rows:
                raise ValueError(f"mask {i} holds {m.numel()} words, {old_rows} rows need {(old_rows + 31) // 32}")
        dev = torch.device("cuda", self.device)
        n, grown = len(masks), (new_rows - old_rows if fill else 0)
        if counts is None:
            bounds = [new_rows] * n
        else:  # a removal only takes rows away; an insertion adds exactly the new rows, where they are set
            bounds = [min(int(c) + grown, new_rows) for c in counts]
        outs = [torch.empty((new_rows + 31) // 32, dtype=torch.int32, device=dev) for _ in masks]
        lists = [torch.empty(b, dtype=torch.int32, device=dev) for b in bounds]
        in_ptrs = (c_void_p * n)(*[m.data_ptr() if m.numel() else None for m in masks])
        out_ptrs = (c_void_p * n)(*[o.data_ptr() if o.numel() else None for o in outs])
        list_ptrs = (c_void_p * n)(*[r.data_ptr() if r.numel() else None for r in lists])
        caps = (c_int64 * n)(*bounds)
        infos = (MaskInfo * n)()
        torch.cuda.current_stream(self.device).synchronize()  # whatever produced the masks (and the allocations above) ran on torch's stream
        with self._lock:
            rc = self.lib.tavb_mask_remap(self._h, mode, c_void_p(dev_flags.data_ptr()) if flag_rows else None, old_rows, new_rows, in_ptrs, out_ptrs, n,
                                          int(fill), list_ptrs, caps, infos)
        _check(self.lib, rc)
        result = []
        for out, rows_out, bound, info in zip(outs, lists, bounds, infos):
            cnt = int(info.count)
            dev_rows = rows_out[:cnt].clone() if bound > 2 * cnt else rows_out[:cnt]
            result.append((dev_rows, cnt, out, (int(info.first_row), int(info.last_row)) if cnt else None))
        return result

    def search_messages_masked(self, queries, dev_bits, dev_rows, k: int, thrs, max_messages: int, route: int, span=None):
        """A masked batch aggregated to messages in one submission (tavb_search_messages_masked): the arguments of `search_masked_wide`
        plus `route` -- 1 = the row list, 2 = the 32/64-query tile, 3 = the 128/256-query filter tile + rescoring; TavbError
        (TAVB_E_UNSUPPORTED) for a shape the route does not serve -- and max_messages; 1 <= k <= 256 -> (message ordinals [nq, k], scores
        [nq, k], counts [nq]).  Per query: `search_messages(q, k, thr, max_messages, subset_rows=the mask's rows)`."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        bits, first, last = self._masked_args(dev_bits, span)
        rows_ptr, n_allowed = (None, 0) if dev_rows is None else self._row_list(dev_rows)
        with self._lock:
            rc = self.lib.tavb_search_messages_masked(self._h, _addr(a), nq, bits, int(self.rows), first, last, rows_ptr, n_allowed, k, _addr(t),
                                                      int(max_messages), int(route), _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    # scoped batches: one mask per query ---------------------------------------------------
    def _mask_pointers(self, dev_bits_list, n: int):
        """n packed masks (torch int32 [(rows + 31) // 32] on this device, repeats allowed) -> the host array of their device pointers the
        scoped calls take (tavb_mask_combine's convention)."""
        torch = self._torch
        masks = list(dev_bits_list)
        if len(masks) != n:
            raise ValueError(f"{len(masks)} masks for {n} queries")
        for i, m in enumerate(masks):
            if not isinstance(m, torch.Tensor) or m.dtype != torch.int32:
                raise TypeError(f"mask {i} must be a torch int32 tensor of packed words")
            if m.dim() != 1 or not m.is_contiguous() or m.numel() * 32 < self.rows:
                raise ValueError(f"mask {i} must be a contiguous 1-D tensor of at least {(self.rows + 31) // 32} words (the corpus has {self.rows} rows)")
            if not m.is_cuda or (m.device.index or 0) != self.device:
                raise ValueError(f"mask {i} must live on cuda:{self.device}")
        return (c_void_p * max(n, 1))(*[m.data_ptr() for m in masks])

    def search_scoped_batch(self, queries, dev_bits_list, k: int, thrs):
        """A batch whose queries carry their own scopes, in one submission (tavb_search_scoped_batch): queries f32 [nq, dim];
        dev_bits_list: nq packed masks on this device, one per query; 1 <= k <= 256; thrs float32 [nq] (or one for all) -> (ordinals
        [nq, k], scores [nq, k], counts [nq]), per query `search_subset_batch_resident` over that mask's row list, bit for bit."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_scoped_batch(self._h, _addr(a), nq, ptrs, int(self.rows), k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_scoped_device(self, dev_queries, dev_bits_list, k: int, thrs, out_keys=None):
        """`search_scoped_batch` with the queries on the device (tavb_search_scoped_device): dev_queries torch f32 [nq, dim] -> torch int64
        [nq, k] sorted, zero-padded keys carrying ordinal_base + row.  `out_keys`: a device tensor or a PINNED host tensor.  The call
        waits for the unions' counts only: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_scoped_device(self._h, c_void_p(dev_queries.data_ptr()), nq, ptrs, int(self.rows), k, _addr(t), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_scoped_topk(self, queries, dev_bits_list, k: int, thrs):
        """`search_scoped_batch` for any 1 <= k <= MAX_LARGE_K, in one submission (tavb_search_scoped_topk): the exact device top-k's
        score pass over the union list of every pass of eight queries, a row scored for a query only inside that query's scope ->
        (ordinals [nq, k], scores [nq, k], counts [nq]), per query `search_subset_batch_resident` over that mask's row list, bit for bit."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_scoped_topk(self._h, _addr(a), nq, ptrs, int(self.rows), k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_scoped_topk_device(self, dev_queries, dev_bits_list, k: int, thrs, out_keys=None):
        """`search_scoped_topk` with the queries on the device (tavb_search_scoped_topk_device) -> torch int64 [nq, k] sorted, zero-padded
        keys carrying ordinal_base + row.  `out_keys`: a device tensor or a PINNED host tensor.  The call waits for the unions' sizes
        only: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_scoped_topk_device(self._h, c_void_p(dev_queries.data_ptr()), nq, ptrs, int(self.rows), k, _addr(t),
                                                         c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def _sorted_batch(self, a, k: int, thrs, max_total: int, call):
        """The arguments and outputs of a sorted batch of the queries a (`batch_queries`): `call(queries, nq, thresholds, max_total,
        ordinals, scores, counts, total)` under the lock -> (ordinals int64 [total], scores float32 [total], counts int64 [nq]), query
        q's results at counts[:q].sum() .. ."""
        if k < 0 or max_total < 0:
            raise ValueError("k and max_total must be >= 0")
        nq = a.shape[0]
        t = batch_thresholds(thrs, nq)
        ords = np.empty(max(max_total, 1), dtype=np.int64)  # (lazy: only the pages the results touch are ever mapped)
        scs = np.empty(max(max_total, 1), dtype=np.float32)
        cnts = np.zeros(nq, dtype=np.int64)
        total = c_int64(0)
        with self._lock:
            rc = call(_addr(a), nq, _addr(t), int(max_total), _addr(ords), _addr(scs), _addr(cnts), byref(total))
        _check(self.lib, rc)
        m = int(total.value)
        return ords[:m], scs[:m], cnts

    def search_scoped_sorted(self, queries, dev_bits_list, k: int, thrs, max_total: int):
        """A scoped batch on the sorted route, in one submission (tavb_search_scoped_sorted): k = 0 (every survivor of the query's scope)
        or any k; max_total: the most results the batch may have (more raise TavbError) -- the sum of min(k, rows of the scope) bounds
        it.  -> `search_sorted`'s layout with corpus ordinals; per query `search_subset_sorted` over that mask's row list, bit for bit."""
        a = batch_queries(queries, self.dim)
        ptrs = self._mask_pointers(dev_bits_list, a.shape[0])
        return self._sorted_batch(a, k, thrs, max_total, lambda qa, nq, t, bound, *out: self.lib.tavb_search_scoped_sorted(
            self._h, qa, nq, ptrs, int(self.rows), int(k), t, bound, *out))

    def search_subset_batch_sorted(self, queries, dev_rows, k: int, thrs):
        """`search_subset_sorted` for a batch over ONE resident row list (tavb_search_subset_batch_sorted), with corpus ordinals
        (dev_rows ascending: `mask_to_rows`) -> `search_sorted`'s layout."""
        a = batch_queries(queries, self.dim)
        rows_ptr, n = self._row_list(dev_rows)
        bound = a.shape[0] * (n if k <= 0 else min(int(k), n))
        return self._sorted_batch(a, k, thrs, bound, lambda qa, nq, t, bound, *out: self.lib.tavb_search_subset_batch_sorted(
            self._h, qa, nq, rows_ptr, n, int(k), t, bound, *out))

    def search_top_messages(self, queries, k: int, thrs, dev_rows=None):
        """The best k MESSAGES of every query -- per message the best score of its rows that pass the threshold, then the top k, all on the
        device (tavb_search_top_messages): queries f32 [nq, dim]; thrs float32 [nq] (or one for all); 1 <= k <= MAX_LARGE_K; dev_rows: a
        resident row list (torch int32 [S], valid corpus rows, e.g. `mask_to_rows`) to search instead of the whole corpus -> (message
        ordinals [nq, k], scores [nq, k], counts [nq]).  Needs `set_row_messages` over exactly the corpus' rows."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        rows_ptr, n = (None, 0) if dev_rows is None else self._row_list(dev_rows)
        if dev_rows is not None and n == 0:  # (an empty tensor has no address to name "a list" by)
            return msgs, scs, cnts
        with self._lock:
            rc = self.lib.tavb_search_top_messages(self._h, _addr(a), nq, k, _addr(t), rows_ptr, n, _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    def search_top_messages_device(self, dev_queries, k: int, thrs, out_keys=None, dev_rows=None):
        """`search_top_messages` with the queries on the device and nothing waited for (tavb_search_top_messages_device): dev_queries torch
        f32 [nq, dim] -> torch int64 [nq, k] sorted, zero-padded keys carrying MESSAGE ordinals (`decode_keys`).  `out_keys`: a device
        tensor or a PINNED host tensor.  Async: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        rows_ptr, n = (None, 0) if dev_rows is None else self._row_list(dev_rows)
        if dev_rows is not None and n == 0:
            self.synchronize()
            out_keys.view(-1)[: nq * k].zero_()
            self._torch.cuda.current_stream(self.device).synchronize()
            return out_keys
        with self._lock:
            rc = self.lib.tavb_search_top_messages_device(self._h, c_void_p(dev_queries.data_ptr()), nq, k, _addr(t), rows_ptr, n,
                                                          c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    plan_top_messages_tile = staticmethod(plan_top_messages_tile)

    def _tile_mask_args(self, dev_bits, span):
        """(dev_bits pointer or None, rows, first, last) of the top-messages tile calls: None = the whole corpus."""
        if dev_bits is None:
            return None, int(self.rows), 0, int(self.rows) - 1
        bits, first, last = self._masked_args(dev_bits, span)
        return bits, int(self.rows), first, last

    def search_top_messages_tile(self, queries, k: int, thrs, dev_bits=None, span=None):
        """`search_top_messages` on the 32/64-query MFMA tile (tavb_search_top_messages_tile): one corpus pass per 64 queries instead of one
        per eight; dev_bits: ONE packed mask (torch int32 [(rows + 31) // 32] on this device, `mask_to_rows_bits`) with span = (first,
        last) allowed row, or None for the whole corpus; 1 <= k <= MAX_LARGE_K -> (message ordinals [nq, k], scores [nq, k], counts
        [nq]).  Scores are the tile's own -- within a few ulp of `search_top_messages`', not bit for bit.  Raises TavbError
        (TAVB_E_UNSUPPORTED) for rows that are not a multiple of 64 bytes."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        bits, rows, first, last = self._tile_mask_args(dev_bits, span)
        with self._lock:
            rc = self.lib.tavb_search_top_messages_tile(self._h, _addr(a), nq, k, _addr(t), bits, rows, first, last, _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    def search_top_messages_tile_device(self, dev_queries, k: int, thrs, out_keys=None, dev_bits=None, span=None):
        """`search_top_messages_tile` with the queries on the device (tavb_search_top_messages_tile_device) -> torch int64 [nq, k] sorted,
        zero-padded keys carrying MESSAGE ordinals (`decode_keys`).  `out_keys`: a device tensor or a PINNED host tensor.  Async:
        `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        bits, rows, first, last = self._tile_mask_args(dev_bits, span)
        with self._lock:
            rc = self.lib.tavb_search_top_messages_tile_device(self._h, c_void_p(dev_queries.data_ptr()), nq, k, _addr(t), bits, rows, first, last,
                                                               c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_top_messages_scoped(self, queries, dev_bits_list, k: int, thrs):
        """`search_top_messages` under one scope PER QUERY, in one submission (tavb_search_top_messages_scoped): dev_bits_list: nq packed
        masks on this device, one per query; per pass of eight queries one scan of the union of their scopes that raises a message's
        best score for a query only inside that query's scope -> (message ordinals [nq, k], scores [nq, k], counts [nq]), per query
        `search_top_messages` over that mask's row list, bit for bit."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_top_messages_scoped(self._h, _addr(a), nq, ptrs, int(self.rows), k, _addr(t), _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    def search_top_messages_scoped_device(self, dev_queries, dev_bits_list, k: int, thrs, out_keys=None):
        """`search_top_messages_scoped` with the queries on the device (tavb_search_top_messages_scoped_device) -> torch int64 [nq, k]
        sorted, zero-padded keys carrying MESSAGE ordinals (`decode_keys`).  `out_keys`: a device tensor or a PINNED host tensor.  The
        call waits for the unions' sizes only: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_top_messages_scoped_device(self._h, c_void_p(dev_queries.data_ptr()), nq, ptrs, int(self.rows), k, _addr(t),
                                                                 c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_messages_scoped(self, queries, dev_bits_list, k: int, thrs, max_messages: int):
        """`search_scoped_batch` aggregated to messages in one submission (tavb_search_messages_scoped) -> (message ordinals [nq, k], scores
        [nq, k], counts [nq]); per query `search_messages_masked` on route 1 over that mask."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        with self._lock:
            rc = self.lib.tavb_search_messages_scoped(self._h, _addr(a), nq, ptrs, int(self.rows), k, _addr(t), int(max_messages), _addr(msgs), _addr(scs),
                                                      _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    # scoped batches on the 32/64-query tile ----------------------------------------------
    plan_scoped = staticmethod(plan_scoped)

    def _scope_span(self, span):
        return (0, int(self.rows) - 1) if span is None else (int(span[0]), int(span[1]))

    def search_scoped_tile(self, queries, dev_bits_list, k: int, thrs, span=None):
        """A scoped batch on the 32/64-query MFMA tile (tavb_search_scoped_tile): the arguments of `search_scoped_batch` plus span = (first,
        last) row of the union of the scopes (None: the whole corpus); 1 <= k <= 64 -> (ordinals [nq, k], scores [nq, k], counts [nq]).
        The tile's contract: per query `search_scoped_batch`'s answer except among float32 near-ties.  Raises TavbError
        (TAVB_E_UNSUPPORTED) for a shape the tile does not serve."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_scoped_tile(self._h, _addr(a), nq, ptrs, int(self.rows), first, last, k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_scoped_tile_device(self, dev_queries, dev_bits_list, k: int, thrs, span=None, out_keys=None):
        """`search_scoped_tile` with the queries on the device (tavb_search_scoped_tile_device) -> torch int64 [nq, k] sorted, zero-padded
        keys carrying ordinal_base + row; nothing is waited for: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_scoped_tile_device(self._h, c_void_p(dev_queries.data_ptr()), nq, ptrs, int(self.rows), first, last, k, _addr(t),
                                                         c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_messages_scoped_tile(self, queries, dev_bits_list, k: int, thrs, max_messages: int, span=None):
        """`search_scoped_tile` aggregated to messages in one submission (tavb_search_messages_scoped_tile) -> (message ordinals [nq, k],
        scores [nq, k], counts [nq])."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_messages_scoped_tile(self._h, _addr(a), nq, ptrs, int(self.rows), first, last, k, _addr(t), int(max_messages),
                                                           _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    # scoped batches on the 128/256-query filter tile + rescoring ---------------------------
    plan_scoped_wide = staticmethod(plan_scoped_wide)

    def search_scoped_wide(self, queries, dev_bits_list, k: int, thrs, span=None):
        """A scoped batch on the 128/256-query filter tile + exact rescoring (tavb_search_scoped_wide): the arguments of
        `search_scoped_tile`; fp16 corpora, 1 <= k <= 256 -> (ordinals [nq, k], scores [nq, k], counts [nq]), `search_scoped_batch`'s
        answer bit for bit.  Raises TavbError (TAVB_E_UNSUPPORTED) for a shape the route does not serve."""
        a, nq, t, ords, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_scoped_wide(self._h, _addr(a), nq, ptrs, int(self.rows), first, last, k, _addr(t), _addr(ords), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return ords, scs, cnts

    def search_scoped_wide_device(self, dev_queries, dev_bits_list, k: int, thrs, span=None, out_keys=None):
        """`search_scoped_wide` with the queries on the device (tavb_search_scoped_wide_device) -> torch int64 [nq, k] sorted, zero-padded
        keys carrying ordinal_base + row; `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_scoped_wide_device(self._h, c_void_p(dev_queries.data_ptr()), nq, ptrs, int(self.rows), first, last, k, _addr(t),
                                                         c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_messages_scoped_wide(self, queries, dev_bits_list, k: int, thrs, max_messages: int, span=None):
        """`search_scoped_wide` aggregated to messages in one submission (tavb_search_messages_scoped_wide) -> (message ordinals [nq, k],
        scores [nq, k], counts [nq])."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        ptrs = self._mask_pointers(dev_bits_list, nq)
        first, last = self._scope_span(span)
        with self._lock:
            rc = self.lib.tavb_search_messages_scoped_wide(self._h, _addr(a), nq, ptrs, int(self.rows), first, last, k, _addr(t), int(max_messages),
                                                           _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    def scope_planes(self, dev_bits_list, span=None):
        """The membership planes of a scoped batch on the tile (tavb_scope_planes): torch int32 [blocks, words] on the device, shaped by
        `scope_plane_shape` -- bit i of [b, r - first // 256 * 256] = mask 32 b + i holds row r.  Async on the engine's stream."""
        torch = self._torch
        masks = list(dev_bits_list)
        ptrs = self._mask_pointers(masks, len(masks))
        first, last = self._scope_span(span)
        blocks, words, _ = scope_plane_shape(len(masks), first, last)
        out = torch.empty((blocks, max(words, 0)), dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.current_stream(self.device).synchronize()
        with self._lock:
            rc = self.lib.tavb_scope_planes(self._h, ptrs, len(masks), int(self.rows), first, last, c_void_p(out.data_ptr()) if out.numel() else None)
        _check(self.lib, rc)
        return out

    def mask_membership(self, dev_bits_list, dev_rows):
        """Which of 1 .. 8 packed masks hold each row of a resident row list (tavb_mask_membership): torch uint8 [S] on the device, bit j of
        byte p = mask j holds row dev_rows[p] -- what a scoped pass reads per row of its union.  Async on the engine's stream."""
        torch = self._torch
        masks = list(dev_bits_list)
        if not 1 <= len(masks) <= MAX_MASK_OPERANDS:
            raise ValueError(f"a membership test has 1 .. {MAX_MASK_OPERANDS} masks (got {len(masks)})")
        ptrs = self._mask_pointers(masks, len(masks))
        rows_ptr, n = self._row_list(dev_rows)
        out = torch.empty(n, dtype=torch.uint8, device=dev_rows.device)
        torch.cuda.current_stream(self.device).synchronize()
        with self._lock:
            rc = self.lib.tavb_mask_membership(self._h, ptrs, len(masks), int(self.rows), rows_ptr, n, c_void_p(out.data_ptr()) if n else None)
        _check(self.lib, rc)
        return out

    def search_messages_batch(self, queries, k: int, thrs, max_messages: int, accept=None):
        """`search_messages` for a batch in one submission (tavb_search_messages_batch): queries f32 [nq, dim]; thrs float32 [nq] (or one
        for all); accept as there -> (message ordinals [nq, k], scores [nq, k], counts [nq])."""
        a, nq, t, msgs, scs, cnts = self._host_batch(queries, k, thrs)
        acc = None if accept is None else np.ascontiguousarray(accept, dtype=np.int32)
        with self._lock:
            rc = self.lib.tavb_search_messages_batch(self._h, _addr(a), nq, k, _addr(t), _addr(acc) if acc is not None and acc.size else None,
                                                     -1 if acc is None else acc.shape[0], int(max_messages), _addr(msgs), _addr(scs), _addr(cnts))
        _check(self.lib, rc)
        return msgs, scs, cnts

    # split form (several contexts driven from one thread) --------------------
    def search_begin(self, queries: np.ndarray, k: int, thrs: np.ndarray, cursor_key: int | None = None) -> None:
        """queries f32 [nq, dim] (contiguous), thrs f32 [nq]: enqueue; pair with search_end(nq, k)."""
        cur = None
        if cursor_key is not None:
            cur = (c_uint64 * 1)(int(cursor_key))
        with self._lock:
            rc = self.lib.tavb_search_begin(self._h, _addr(queries), queries.shape[0], k, _addr(thrs),
                                            ctypes.cast(cur, c_void_p) if cur is not None else None)
        _check(self.lib, rc)

    def search_end(self, nq: int, k: int, out_keys: np.ndarray) -> None:
        """out_keys: uint64 [nq, k] (contiguous) <- sorted key lists with global ordinals."""
        with self._lock:
            rc = self.lib.tavb_search_end(self._h, nq, k, _addr(out_keys))
        _check(self.lib, rc)

    # device-resident forms ---------------------------------------------------
    def _check_out_keys(self, out_keys, nq: int, k: int) -> None:
        """The kernels write nq * k keys at out_keys.data_ptr(), row q at q * k: anything but a contiguous int64 tensor of at least that many
        elements, in this device's memory or in pinned host memory (which the device writes directly), is refused before any launch."""
        torch = self._torch
        if not isinstance(out_keys, torch.Tensor) or out_keys.dtype != torch.int64:
            raise ValueError("out_keys must be an int64 torch tensor")
        if not out_keys.is_contiguous():
            raise ValueError("out_keys must be contiguous (the kernels write row q of the result at q * k)")
        if out_keys.numel() < nq * k:
            raise ValueError(f"out_keys holds {out_keys.numel()} keys; this lookup writes {nq} x {k} = {nq * k}")
        dev = out_keys.device
        on_device = dev.type == "cuda" and (dev.index if dev.index is not None else torch.cuda.current_device()) == self.device
        if not on_device and not (dev.type == "cpu" and out_keys.is_pinned()):
            raise ValueError(f"out_keys must live on cuda:{self.device} or in pinned host memory")

    def _out_keys(self, out_keys, nq: int, k: int, device):
        """The caller's `out_keys`, checked, or a fresh torch int64 [nq, k] on `device`."""
        if out_keys is None:
            out_keys = self._torch.empty((nq, k), dtype=self._torch.int64, device=device)
        self._check_out_keys(out_keys, nq, k)
        return out_keys

    def _device_batch(self, dev_queries, k: int, thrs, out_keys, flat: bool = False):
        """The arguments of a lookup whose queries are on the device: dev_queries torch f32 [nq, dim] (flat: any shape of nq * dim
        elements) -> (nq, thresholds f32 [nq] -- None for thrs=None: the forms that pass one scalar threshold --, `_out_keys`)."""
        assert dev_queries.dtype == self._torch.float32 and dev_queries.is_contiguous()
        if flat:
            assert dev_queries.numel() % max(self.dim, 1) == 0
            nq = dev_queries.numel() // self.dim if self.dim else 0
        else:
            assert dev_queries.dim() == 2 and dev_queries.shape[1] == self.dim
            nq = int(dev_queries.shape[0])
        t = None if thrs is None else batch_thresholds(thrs, nq)
        return nq, t, self._out_keys(out_keys, nq, k, dev_queries.device)

    def search_device(self, dev_queries, k: int, thr: float, out_keys=None):
        """dev_queries: torch f32 [nq, dim] on this device -> torch int64 [nq, k] of packed keys (async)."""
        nq, _, out_keys = self._device_batch(dev_queries, k, None, out_keys)
        with self._lock:
            rc = self.lib.tavb_search_device(self._h, c_void_p(dev_queries.data_ptr()), nq, k, c_float(float(thr)), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_topk_device(self, dev_queries, k: int, thrs, out_keys=None, dev_rows=None):
        """`search_topk` / `search_subset_topk` with the queries on the device and nothing waited for (tavb_search_topk_device): dev_queries
        torch f32 [nq, dim]; thrs float32 [nq] (or one for all); 1 <= k <= MAX_LARGE_K -> torch int64 [nq, k] sorted, zero-padded keys
        carrying global ordinals -- or, with dev_rows (torch int32 [S], valid corpus rows; one query), subset positions.  `out_keys`: a
        device tensor or a PINNED host tensor.  Async: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys, flat=True)  # (flat: one query may come as [dim])
        rows_ptr, n_rows = (None, 0) if dev_rows is None else self._row_list(dev_rows)
        if dev_rows is not None and n_rows == 0:  # (an empty tensor has no address to tell the library "a subset" by)
            self.synchronize()
            out_keys.view(-1)[: nq * k].zero_()
            self._torch.cuda.current_stream(self.device).synchronize()
            return out_keys
        with self._lock:
            rc = self.lib.tavb_search_topk_device(self._h, c_void_p(dev_queries.data_ptr()), nq, k, _addr(t), rows_ptr, n_rows, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_subset_batch_device(self, dev_queries, dev_rows, k: int, thrs, out_keys=None, remap: bool = True):
        """`search_subset_batch_resident` with the queries on the device and nothing waited for (tavb_search_subset_batch_device):
        dev_queries torch f32 [nq, dim], nq >= 1, over ONE resident row list (torch int32 [S]: `mask_to_rows`, or wrapped, range-checked
        rows); thrs float32 [nq] (or one for all); 1 <= k <= MAX_LARGE_K -> torch int64 [nq, k] sorted, zero-padded keys.  remap=True:
        the keys carry global ordinals (ordinal_base + row: what the key merges take; dev_rows ascending); False: positions in dev_rows.
        `out_keys`: a device tensor or a PINNED host tensor.  Async: `synchronize()` before reading."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        rows_ptr, n = self._row_list(dev_rows)
        with self._lock:  # (an empty tensor has no address to name "a subset" by: length 0 and no pointer -- the library enqueues zero keys)
            rc = self.lib.tavb_search_subset_batch_device(self._h, c_void_p(dev_queries.data_ptr()), nq, rows_ptr, n,
                                                          k, _addr(t), 1 if remap else 0, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_subset_device(self, dev_query, dev_rows, k: int, thr: float, out_keys=None):
        """dev_query: torch f32 [1, dim] or [dim]; dev_rows: torch int32 [S] (valid corpus rows) ->
        torch int64 [1, k] packed keys carrying subset positions (async)."""
        torch = self._torch
        assert dev_query.dtype == torch.float32 and dev_query.is_contiguous() and dev_query.numel() == self.dim
        assert dev_rows.dtype == torch.int32 and dev_rows.is_contiguous() and dev_rows.dim() == 1
        out_keys = self._out_keys(out_keys, 1, k, dev_query.device)
        with self._lock:
            rc = self.lib.tavb_search_subset_device(self._h, c_void_p(dev_query.data_ptr()), c_void_p(dev_rows.data_ptr()),
                                                    dev_rows.shape[0], k, c_float(float(thr)), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    # row shards, one process per GPU: the library's own RCCL communicator ----------------------------------
    def comm_init(self, unique_id: bytes, rank: int, world: int) -> None:
        """Collective over all ranks: join the communicator named by `unique_id` (from `comm_unique_id()` on rank 0)."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"the rendezvous id is {COMM_ID_BYTES} bytes")
        buf = ctypes.create_string_buffer(bytes(unique_id), COMM_ID_BYTES)
        with self._lock:
            rc = self.lib.tavb_comm_init(self._h, ctypes.cast(buf, c_void_p), int(rank), int(world))
        _check(self.lib, rc)

    def comm_destroy(self) -> None:
        with self._lock:
            rc = self.lib.tavb_comm_destroy(self._h)
        _check(self.lib, rc)

    def search_allgather(self, dev_queries, k: int, thr: float, out_keys=None):
        """Collective `search_device`: every rank passes the same queries and gets the merged whole-corpus key lists [nq, k].
        `out_keys`: a device tensor or a PINNED host tensor (int64 [nq, k]; the merge kernel writes it directly).  Async."""
        nq, _, out_keys = self._device_batch(dev_queries, k, None, out_keys)
        with self._lock:
            rc = self.lib.tavb_search_allgather(self._h, c_void_p(dev_queries.data_ptr()), nq, k, c_float(float(thr)), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def allgather_merge(self, dev_local_keys, out_keys=None):
        """Collective: this rank's sorted lists [nq, k] (global ordinals / positions) -> the lists merged over all ranks (async)."""
        torch = self._torch
        assert dev_local_keys.dtype == torch.int64 and dev_local_keys.is_contiguous() and dev_local_keys.dim() == 2
        nq, k = dev_local_keys.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_local_keys.device)
        with self._lock:
            rc = self.lib.tavb_allgather_merge(self._h, c_void_p(dev_local_keys.data_ptr()), nq, k, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_topk_allgather(self, dev_queries, k: int, thrs, out_keys=None):
        """Collective `search_topk_device` (tavb_search_topk_allgather): every rank passes the same queries and thresholds and gets the
        merged whole-corpus key lists [nq, k], 1 <= k <= MAX_LARGE_K.  `out_keys`: a device tensor or a PINNED host tensor.  Async."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        with self._lock:
            rc = self.lib.tavb_search_topk_allgather(self._h, c_void_p(dev_queries.data_ptr()), nq, k, _addr(t), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def allgather_merge_topk(self, dev_local_keys, out_keys=None):
        """`allgather_merge` for lists of up to MAX_LARGE_K keys (tavb_allgather_merge_topk).  Async; collective."""
        torch = self._torch
        assert dev_local_keys.dtype == torch.int64 and dev_local_keys.is_contiguous() and dev_local_keys.dim() == 2
        nq, k = dev_local_keys.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_local_keys.device)
        with self._lock:
            rc = self.lib.tavb_allgather_merge_topk(self._h, c_void_p(dev_local_keys.data_ptr()), nq, k, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def search_top_messages_allgather(self, dev_queries, k: int, thrs, out_keys=None, dev_rows=None):
        """Collective `search_top_messages_device` (tavb_search_top_messages_allgather): every rank passes the same queries and thresholds
        and gets the merged whole-corpus lists [nq, k] of keys carrying MESSAGE ordinals, 1 <= k <= MAX_LARGE_K.  dev_rows: None -- this
        rank's whole shard -- or this rank's part of a mask as shard-local rows (torch int32 [S]; an EMPTY tensor: this rank joins with
        zero lists).  Needs `set_row_messages` with the same n_messages on every rank.  `out_keys`: a device tensor or a PINNED host tensor.
        Async."""
        nq, t, out_keys = self._device_batch(dev_queries, k, thrs, out_keys)
        rows_ptr, n = (None, 0) if dev_rows is None else self._row_list(dev_rows)
        if dev_rows is not None and n == 0:  # (an empty tensor has no address: any non-null pointer names "an empty part of a mask")
            rows_ptr = c_void_p(dev_queries.data_ptr())
        with self._lock:
            rc = self.lib.tavb_search_top_messages_allgather(self._h, c_void_p(dev_queries.data_ptr()), nq, k, _addr(t), rows_ptr, n,
                                                             c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def allgather_merge_top_messages(self, dev_local_keys, out_keys=None):
        """`allgather_merge_topk` for lists whose keys carry MESSAGE ordinals (tavb_allgather_merge_top_messages): per message the largest
        key over all ranks, then the best k.  Async; collective."""
        torch = self._torch
        assert dev_local_keys.dtype == torch.int64 and dev_local_keys.is_contiguous() and dev_local_keys.dim() == 2
        nq, k = dev_local_keys.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_local_keys.device)
        with self._lock:
            rc = self.lib.tavb_allgather_merge_top_messages(self._h, c_void_p(dev_local_keys.data_ptr()), nq, k, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def remap_key_positions(self, dev_keys, dev_map) -> None:
        """In place: keys carrying list positions -> keys carrying dev_map[position] (int32 device tensor).  Async."""
        torch = self._torch
        assert dev_keys.dtype == torch.int64 and dev_keys.is_contiguous() and dev_map.dtype == torch.int32 and dev_map.is_contiguous()
        with self._lock:
            rc = self.lib.tavb_remap_key_positions(self._h, c_void_p(dev_keys.data_ptr()), dev_keys.numel(), c_void_p(dev_map.data_ptr()), dev_map.numel())
        _check(self.lib, rc)

    def merge_device(self, dev_lists, out_keys=None):
        """dev_lists: torch int64 [n_lists, nq, k] -> [nq, k] (async)."""
        torch = self._torch
        assert dev_lists.dtype == torch.int64 and dev_lists.is_contiguous() and dev_lists.dim() == 3
        n_lists, nq, k = dev_lists.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_lists.device)
        with self._lock:
            rc = self.lib.tavb_merge_device(self._h, c_void_p(dev_lists.data_ptr()), n_lists, nq, k, c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def merge_topk_device(self, dev_lists, out_keys=None, query_major: bool = False):
        """`merge_device` for lists of up to MAX_LARGE_K keys (tavb_merge_topk_device): dev_lists torch int64 [n_lists, nq, k] -- or
        [nq, n_lists, k] with query_major -- of sorted, zero-padded lists with unique keys, n_lists <= 64 -> [nq, k] (async)."""
        torch = self._torch
        assert dev_lists.dtype == torch.int64 and dev_lists.is_contiguous() and dev_lists.dim() == 3
        if query_major:
            nq, n_lists, k = dev_lists.shape
        else:
            n_lists, nq, k = dev_lists.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_lists.device)
        with self._lock:
            rc = self.lib.tavb_merge_topk_device(self._h, c_void_p(dev_lists.data_ptr()), -n_lists if query_major else n_lists, nq, k,
                                                 c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys

    def merge_top_messages_device(self, dev_lists, n_messages: int, out_keys=None, query_major: bool = False):
        """`merge_topk_device` for lists whose keys carry MESSAGE ordinals below n_messages (tavb_merge_top_messages_device): a message may
        stand in several lists -> [nq, k], per message its largest key, the best k, what `merge_top_messages_keys` returns (async)."""
        torch = self._torch
        assert dev_lists.dtype == torch.int64 and dev_lists.is_contiguous() and dev_lists.dim() == 3
        if query_major:
            nq, n_lists, k = dev_lists.shape
        else:
            n_lists, nq, k = dev_lists.shape
        out_keys = self._out_keys(out_keys, nq, k, dev_lists.device)
        with self._lock:
            rc = self.lib.tavb_merge_top_messages_device(self._h, c_void_p(dev_lists.data_ptr()), -n_lists if query_major else n_lists, nq, k,
                                                         int(n_messages), c_void_p(out_keys.data_ptr()))
        _check(self.lib, rc)
        return out_keys


def comm_unique_id() -> bytes:
    """A fresh RCCL rendezvous id (rank 0 creates it and hands it to the other ranks)."""
    lib = load_library()
    buf = ctypes.create_string_buffer(COMM_ID_BYTES)
    _check(lib, lib.tavb_comm_unique_id(ctypes.cast(buf, c_void_p)))
    return buf.raw


def make_key(score: float, ordinal: int) -> int:
    """The packed key of (score, ordinal): (float32 bits << 32) | (0xFFFFFFFF - ordinal)."""
    bits = int(np.float32(score).view(np.uint32))
    return (bits << 32) | (0xFFFFFFFF - int(ordinal))


def merge_keys(lists: np.ndarray) -> np.ndarray:
    """uint64 [n_lists, nq, k] sorted key lists -> uint64 [nq, k] (host k-way merge in libtavb)."""
    lib = load_library(preload_torch=False)
    a = np.ascontiguousarray(lists, dtype=np.uint64)
    n_lists, nq, k = a.shape
    out = np.empty((nq, k), dtype=np.uint64)
    _check(lib, lib.tavb_merge_keys_host(_addr(a), n_lists, nq, k, _addr(out)))
    return out


def merge_topk_keys(lists: np.ndarray) -> np.ndarray:
    """`merge_keys` for lists of up to MAX_LARGE_K keys (tavb_merge_topk_host): uint64 [n_lists <= 64, nq, k] sorted, zero-padded lists with
    unique keys -> uint64 [nq, k]; a query one of whose lists leads with the failure key comes back as that key in every slot.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    a = np.ascontiguousarray(lists).view(np.uint64)
    if a.ndim != 3:
        raise ValueError("lists must be [n_lists, nq, k]")
    n_lists, nq, k = a.shape
    out = np.empty((nq, k), dtype=np.uint64)
    _check(lib, lib.tavb_merge_topk_host(_addr(a), n_lists, nq, k, _addr(out)))
    return out


def merge_top_messages_keys(lists: np.ndarray) -> np.ndarray:
    """`merge_topk_keys` for lists whose keys carry MESSAGE ordinals (tavb_merge_top_messages_host): uint64 [n_lists <= 64, nq, k] sorted,
    zero-padded lists in which one message may stand several times -> uint64 [nq, k]: per message its largest key, the best k, sorted and
    zero-padded; a query one of whose lists leads with the failure key comes back as that key in every slot.  Needs no GPU."""
    lib = load_library(preload_torch=False)
    a = np.ascontiguousarray(lists).view(np.uint64)
    if a.ndim != 3:
        raise ValueError("lists must be [n_lists, nq, k]")
    n_lists, nq, k = a.shape
    out = np.empty((nq, k), dtype=np.uint64)
    _check(lib, lib.tavb_merge_top_messages_host(_addr(a), n_lists, nq, k, _addr(out)))
    return out


def decode_keys(keys: np.ndarray):
    """Host int64/uint64 [nq, k] packed keys -> (ordinals [nq,k], scores [nq,k], counts [nq])."""
    lib = load_library(preload_torch=False)
    a = np.ascontiguousarray(keys).view(np.uint64)
    if a.ndim != 2:
        raise ValueError("keys must be 2-D")
    nq, k = a.shape
    ords = np.empty((nq, k), dtype=np.int64)
    scs = np.empty((nq, k), dtype=np.float32)
    cnts = np.zeros(nq, dtype=np.int32)
    _check(lib, lib.tavb_decode_keys(_addr(a), nq, k, _addr(ords),
                                     _addr(scs), _addr(cnts)))
    return ords, scs, cnts
