"""CPU suite: the large-k entry points of the C ABI (tavb_search_topk, tavb_search_subset_topk) exist, refuse bad arguments without a
GPU, and the binding's constants match include/tavb.h."""

import ctypes
import os
import re

from typeagent_py_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_define(name: str) -> int:
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_constants_match_the_header():
    assert _native.MAX_LARGE_K == header_define("TAVB_MAX_LARGE_K") >= 4096
    assert _native.MAX_LARGE_K > _native.MAX_FUSED_K
    assert _native.KERNEL_TOPK == header_define("TAVB_KERNEL_TOPK") == 9
    assert header_define("TAVB_KERNEL_COUNT") == 10
    assert _native.ABI_VERSION == header_define("TAVB_ABI_VERSION") == 7
    assert {"tavb_search_topk", "tavb_search_subset_topk"} <= set(_native.ABI_SYMBOLS)


def test_null_context_is_refused_without_aborting():
    lib = _native.load_library(preload_torch=False)
    rc = lib.tavb_search_topk(None, None, 1, 1000, None, None, None, None)
    assert rc == -1 and b"null context" in lib.tavb_last_error()
    rc = lib.tavb_search_subset_topk(None, None, None, 10, 1000, ctypes.c_float(0.0), None, None, None)
    assert rc == -1 and b"null context" in lib.tavb_last_error()


def test_options_are_documented():
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    for name in ("large_k", "topk_buckets", "topk_boundary_keys", "topk_scores_bytes", "last_topk_refine"):
        assert f'"{name}"' in text, name
