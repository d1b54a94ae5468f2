"""GPU suite: tavb_set_option / tavb_get_option, one table (a context cannot be created without a device, so this is no CPU test).

OPTIONS was written from the if-chains tavb_set_option and tavb_get_option were before they became one table in csrc/tavb_abi.hip: for every
settable option its default on a fresh context, one accepted value other than the default, and the nearest rejected values on each side.
The checks: get returns the default; set then get round-trips (switches store any non-zero value as 1); a rejected value raises and leaves
the stored value alone; the read-only names can be read and not set; an unknown name raises on both calls; and `f32_shadow = 0` drops the
shadow of an fp32 corpus at once.  By the chains' code everything here held except reading `mfma_sched` and `mfma_ablate`, which could be set
and not read: they have a test of their own (test_measurement_options_can_be_read_back) so that this difference stays visible.

The fault-injection options (comm_fail_rank, comm_fail_alloc, comm_stall_ms) are only set, read back and restored: no call is made to fail.
"""

from __future__ import annotations

import numpy as np
import pytest

from tests.synth import make_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

SWITCH = "switch"  # any value is taken, stored as 0 / 1
BAND_MAX = 2048  # tavb::kBandMax (csrc/tavb_internal.h)
SORT_SMALL_MAX = 16384  # tavb::kSortSmallMax
MAX_GROUPED_QUERIES = 128  # TAVB_MAX_GROUPED_QUERIES

# name: (default, accepted value, rejected values)
OPTIONS = {
    "scan_blocks": (0, 64, (-1, 65536)),
    "scan_waves": (16, 8, (0, 17)),
    "scan_unroll": (2, 4, (0, 3, 5, 8)),
    "scan_nt": (1, SWITCH, ()),
    "scan_pipe": (0, SWITCH, ()),
    "force_tier": (0, 2, (-1, 4)),
    "mfma_min_batch": (65, 70, (0,)),
    "mfma_min_batch_big": (33, 40, (0,)),
    "mfma_big_bytes": (256 << 20, 0, (-1,)),
    "mfma_min_batch_big_f32": (5, 6, (0,)),
    "mfma_big_bytes_f32": (1_000_000_000, 0, (-1,)),
    "mfma_few_bytes_f32": (4 << 30, 0, (-1,)),
    "mfma_min_batch_f32": (33, 34, (0,)),
    "mfma_sample_rows": (0, -1, (-2,)),
    "f32_shadow": (1, 2, (-1, 3)),
    "f32_shadow_min_bytes": (2 << 30, 0, (-1,)),
    "mfma_tile": (0, 128, (-1, 64, 127, 129, 255, 257, 512)),
    "mfma_sched": (0, 3, (-1, 10)),
    "skinny_min_batch_f32": (5, 1, (0,)),
    "skinny_min_batch_f16": (3, 1, (0,)),
    "mfma_ladder": (4, 0, (-1, 65)),
    "mfma_ablate": (0, 258, (-1, 4096)),
    "mfma_splits": (0, 4096, (-1, 4097)),
    "band_max": (BAND_MAX, _native.MAX_FUSED_K, (_native.MAX_FUSED_K - 1, BAND_MAX + 1)),
    "early_exact": (1, SWITCH, ()),
    "wide_fallback": (1, SWITCH, ()),
    "mfma_bdirect": (0, SWITCH, ()),
    "mfma_shape": (16, 32, (0, 15, 17, 31, 33)),
    "small_direct_keys": (8192, 64, (63, (1 << 20) + 1)),
    "inline_query": (1, SWITCH, ()),
    "direct_group_max_nq": (MAX_GROUPED_QUERIES, 0, (-1, MAX_GROUPED_QUERIES + 1)),
    "direct_group": (0, 8, (-1, 3, 5, 7, 9, 16)),
    "direct_group_wgs": (0, 8, (-1, 1, 7, 65537)),
    "direct_group_keys": (32768, 64, (63, (1 << 22) + 1)),
    "small_direct_bytes": (128 << 20, 0, (-1,)),
    "comm_force": (0, SWITCH, ()),
    "comm_fail_rank": (-1, 3, (-2,)),
    "comm_fail_alloc": (0, SWITCH, ()),
    "comm_stall_ms": (0, 5000, (-1, 5001)),
    "comm_timeout_ms": (0, 100, (-1,)),
    "comm_reserve_keys": (1 << 20, _native.MAX_FUSED_K, (_native.MAX_FUSED_K - 1, (1 << 28) + 1)),
    "graph_max_bytes": (0, 1 << 20, (-1,)),
    "large_k": (1, SWITCH, ()),
    "topk_buckets": (1024, 320, (192, 255, 257, 320 + 1, 4096 + 64)),
    "topk_boundary_keys": (16384, 64, (63, _native.MAX_LARGE_K + 1)),
    "topk_scores_bytes": (1 << 30, 4096, (4095,)),
    "sort_all": (1, SWITCH, ()),
    "sort_stage_keys": (1 << 21, 1, (0, (1 << 30) + 1)),
    "sort_small_keys": (16384, 0, (-1, SORT_SMALL_MAX + 1)),
}
SET_NOT_READ_BEFORE = ("mfma_sched", "mfma_ablate")  # settable, and not readable while the getter was a chain of its own

# name: value on a fresh context (None: whatever the device has)
READ_ONLY = {
    "last_shadow": 0,
    "last_mfma_shape": 0,
    "last_skinny_kernel": 0,
    "last_direct": 0,
    "last_graph": 0,
    "last_topk_refine": 0,
    "last_tier": 0,
    "compute_units": None,
    "last_doomed": 0,
    "last_flagged": 0,
    "comm_world": 0,
    "comm_rank": -1,
}


@pytest.fixture()
def eng(monkeypatch):
    monkeypatch.delenv("TAVB_ENGINE_OPTIONS", raising=False)
    e = _native.Engine(0)
    yield e
    e.close()


def _check_option(eng, name):
    default, accepted, rejected = OPTIONS[name]
    assert eng.get_option(name) == default
    if accepted == SWITCH:
        for v, stored in ((1 - default, 1 - default), (default, default), (7, 1), (-1, 1), (1 << 40, 1), (0, 0)):
            eng.set_option(name, v)
            assert eng.get_option(name) == stored, (name, v)
    else:
        assert accepted != default
        eng.set_option(name, accepted)
        assert eng.get_option(name) == accepted
        for v in rejected:
            with pytest.raises(ValueError):
                eng.set_option(name, v)
            assert eng.get_option(name) == accepted, (name, v)
    eng.set_option(name, default)
    assert eng.get_option(name) == default


@pytest.mark.parametrize("name", [n for n in OPTIONS if n not in SET_NOT_READ_BEFORE])
def test_option_default_round_trip_and_bounds(eng, name):
    _check_option(eng, name)


@pytest.mark.parametrize("name", SET_NOT_READ_BEFORE)
def test_measurement_options_are_set_and_bounded(eng, name):
    """What held for these two before they could be read: an accepted value is taken, the nearest values outside are refused."""
    _, accepted, rejected = OPTIONS[name]
    eng.set_option(name, accepted)
    for v in rejected:
        with pytest.raises(ValueError):
            eng.set_option(name, v)
    eng.set_option(name, 0)


@pytest.mark.parametrize("name", SET_NOT_READ_BEFORE)
def test_measurement_options_can_be_read_back(eng, name):
    """Every settable option is readable (these two were not, while set and get were two chains kept in step by hand)."""
    _check_option(eng, name)


@pytest.mark.parametrize("name", sorted(READ_ONLY))
def test_read_only_names_can_be_read_and_not_set(eng, name):
    fresh = READ_ONLY[name]
    got = eng.get_option(name)
    assert got == fresh if fresh is not None else got >= 8
    for v in (0, 1, got):
        with pytest.raises(ValueError, match="unknown option"):
            eng.set_option(name, v)
    assert eng.get_option(name) == got


def test_every_name_of_the_header_is_in_one_of_the_tables():
    """include/tavb.h documents the options in the comment above tavb_set_option: a name added there has to be added here."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "tavb.h")).read()
    quoted = set(re.findall(r'"([a-z][a-z0-9_]+)"', header))
    known = set(OPTIONS) | set(READ_ONLY)
    assert quoted & known, "the header no longer quotes option names: rewrite this check"
    assert not {n for n in quoted if re.match(r"(scan|mfma|comm|topk|sort|direct|small_direct|last)_", n)} - known


def test_unknown_names_raise_on_both_calls(eng):
    for name in ("", "scan_wave", "scan_waves ", "SCAN_WAVES", "no_such_option"):
        with pytest.raises(ValueError, match="unknown option"):
            eng.set_option(name, 1)
        with pytest.raises(ValueError, match="unknown option"):
            eng.get_option(name)


def test_comm_reserve_keys_is_refused_once_a_communicator_exists(eng):
    """tavb_comm_init sizes the exchange buffers from it: a later change would not be seen."""
    lib = eng.lib
    uid = (_native.ctypes.c_char * _native.COMM_ID_BYTES)()
    if lib.tavb_comm_unique_id(uid) != 0:
        pytest.fail("librccl could not be loaded: " + lib.tavb_last_error().decode())
    eng.set_option("comm_reserve_keys", 4096)
    eng.comm_init(bytes(uid), 0, 1)
    try:
        assert eng.get_option("comm_world") == 1 and eng.get_option("comm_rank") == 0
        with pytest.raises(ValueError, match="comm_reserve_keys"):
            eng.set_option("comm_reserve_keys", 8192)
        assert eng.get_option("comm_reserve_keys") == 4096
    finally:
        eng.comm_destroy()
    assert eng.get_option("comm_world") == 0 and eng.get_option("comm_rank") == -1
    eng.set_option("comm_reserve_keys", 8192)
    assert eng.get_option("comm_reserve_keys") == 8192


def test_f32_shadow_0_drops_the_shadow_of_an_fp32_corpus(eng):
    """A batch of 80 queries on an fp32 corpus filters on the fp16 shadow (last_shadow 1); with `f32_shadow = 0` the next one does not, and
    answers the same rows."""
    import torch

    v, _ = make_corpus(6000, 256, 5)
    q = make_queries(80, 256, 6)
    eng.set_option("direct_group_max_nq", 0)  # (off the grouped one-launch form: this batch is the wide tile's)
    eng.set_corpus_tensor(torch.from_numpy(v).cuda())
    ords, scs, cnts = eng.search_batch(q, 10, np.float32(0.0))
    assert eng.get_option("last_shadow") == 1 and eng.get_option("last_tier") == 4
    eng.set_option("f32_shadow", 0)
    assert eng.get_option("f32_shadow") == 0
    ords0, scs0, cnts0 = eng.search_batch(q, 10, np.float32(0.0))
    assert eng.get_option("last_shadow") == 0 and eng.get_option("last_tier") != 4
    assert cnts.tolist() == cnts0.tolist() == [10] * 80
    assert np.array_equal(ords, ords0)
    eng.set_option("f32_shadow", 1)
    eng.search_batch(q, 10, np.float32(0.0))
    assert eng.get_option("last_shadow") == 1
