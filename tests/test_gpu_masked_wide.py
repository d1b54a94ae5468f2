"""GPU suite: masked batches on the 128/256-query filter tile + exact rescoring (`tavb_search_masked_wide`; the table is
tests/masked_wide_cases.py).

Every run of a case forces the route (`mask_wide = 2`) and one of the four masked kernels (`masked_wide_cases.VARIANTS`; "auto" leaves the tile
to the library) and asserts:
  1. ordinals, float32 score BITS and counts EQUAL the row-list route's on the same engine (`search_subset_batch_resident` over the mask's
     resident row list: what `mask_wide = 0`, `mask_tile = 0` runs) -- the invariant the unmasked wide route keeps against sequential lookups;
  2. every returned ordinal has its bit set; a zero mask inside a non-empty span returns empty lists;
  3. a sample of the queries agrees with the oracle's subset lookup under the float64 referee;
  4. `masked_route` == 3, `last_tier` == 4, `last_mfma_shape` = the variant's, `last_shadow` = 1 exactly for a padded width; the case built
     for it re-runs flagged queries (`last_flagged` >= 1), the others flag none.
Then the device form, the argument checks and the class (`fuzzy_lookup_embeddings_masked`: a handle and a raw mask, `as_arrays`, per-query
thresholds, `mask_wide` 0 / 1 / 2, fp32 corpora and device groups on their old routes).

A mutant run once over this file -- the bit a lane tests taken from its neighbour's row in both forms (`(r_off ^ 1)` in the 32 x 32 form,
`(j ^ 1)` in the 16 x 16 form) -- fails 121 of the 153 tests; the 32 that pass cannot see a swap inside an even/odd row pair (the all-ones, alternating-word,
complementary 80-row-group and empty masks, contiguous ranges with even ends, the last row next to set bits behind the corpus, the argument
checks and the fp32 / device-group routes).
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import masked_wide_cases as mw
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

GETTERS = ("masked_route", "last_tier", "last_mfma_shape", "last_shadow")
SENTINEL = -0x0123456789ABCDEF


def _torch():
    import torch

    return torch


def _bits(words: np.ndarray):
    return _torch().from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _setup(case: mw.Case, variant: str):
    """-> (engine, the corpus tensor, packed mask on the device, the resident row list, its length)"""
    torch = _torch()
    _, store, _ = mw.case_inputs(case)
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*mw.ROUTE_OPTS, *case.opts, *mw.variant_opts(case, variant)):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev)
    bits = _bits(mw.case_words(case, garbage=mw.case_garbage(case)))
    flat = np.flatnonzero(mw.case_mask(case))
    dev_rows = torch.from_numpy(flat.astype(np.int32)).cuda()
    return eng, dev, bits, dev_rows, flat


def _assert_equal_answers(what, got, want):
    (o, s, c), (o2, s2, c2) = got, want
    assert np.array_equal(c, c2), f"{what}: counts differ for queries {np.flatnonzero(c != c2)[:8].tolist()}: {c[c != c2][:8].tolist()} against {c2[c != c2][:8].tolist()}"
    for qi in range(len(c)):
        m = int(c[qi])
        if not np.array_equal(o[qi, :m], o2[qi, :m]):
            only = sorted(set(o[qi, :m].tolist()) ^ set(o2[qi, :m].tolist()))
            raise AssertionError(f"{what}: query {qi}: ordinals differ; in one answer only {only[:12]} (row mod 320: {[r % 320 for r in only[:12]]}, bit "
                                 f"{[r % 32 for r in only[:12]]})")
        assert np.array_equal(s[qi, :m].view(np.uint32), s2[qi, :m].view(np.uint32)), f"{what}: query {qi}: score bits differ"


@pytest.mark.parametrize("case,variant", mw.RUNS, ids=[f"{c.name}-{v}" for c, v in mw.RUNS])
def test_masked_wide_case(case, variant):
    v, store, qs = mw.case_inputs(case)
    mask = mw.case_mask(case)
    eng, dev, bits, dev_rows, flat = _setup(case, variant)
    thrs = mw.case_thresholds(case)
    what = f"{case.name} {variant}"
    span = mw.case_span(case)
    if span is None:  # a zero mask inside a non-empty span: the filter runs and admits nothing
        assert eng.search_masked_wide(qs, bits, dev_rows, case.k, thrs, span=(0, case.rows - 1))[2].tolist() == [0] * case.nq  # an empty row list: no launch
        one_row = _torch().zeros(1, dtype=_torch().int32, device="cuda")  # a row list that names row 0 although its bit is clear: only the re-run would read it
        got = eng.search_masked_wide(qs, bits, one_row, case.k, thrs, span=(0, case.rows - 1))
        assert got[2].tolist() == [0] * case.nq, f"{what}: a zero mask returned rows"
        state = {g: eng.get_option(g) for g in GETTERS}
        assert state == {"masked_route": 3, "last_tier": 4, "last_mfma_shape": mw.variant_shape(case, variant), "last_shadow": 0}, (what, state)
        eng.close()
        return
    want = eng.search_subset_batch_resident(qs, dev_rows, case.k, thrs, remap=True)
    assert eng.get_option("masked_route") == 1
    got = eng.search_masked_wide(qs, bits, dev_rows, case.k, thrs, span=span)
    state = {g: eng.get_option(g) for g in GETTERS}
    assert state == {"masked_route": 3, "last_tier": 4, "last_mfma_shape": mw.variant_shape(case, variant), "last_shadow": int(case.padded)}, (what, state)
    flagged = eng.get_option("last_flagged")
    if case.dups:
        assert flagged >= 1, f"{what}: no query was flagged, the re-run did not happen"
    else:
        assert flagged == 0, f"{what}: {flagged} queries flagged"
    ords, scs, cnts = got
    for qi in range(case.nq):
        bad = [int(o) for o in ords[qi, : cnts[qi]] if not (0 <= o < case.rows and mask[o])]
        assert not bad, f"{what}: query {qi} returned disallowed rows {bad[:12]} (row mod 320: {[r % 320 for r in bad[:12]]})"
    _assert_equal_answers(what, got, want)
    dead = np.isnan(thrs) | (thrs > 1)
    assert (cnts[dead] == 0).all()
    if case.thr == "zero":
        assert (cnts == min(case.k, len(flat))).all(), f"{what}: counts {np.unique(cnts).tolist()}"
    sub = v[flat]
    for qi in sorted({0, 1, 5, 17, case.nq // 2, case.nq - 2, case.nq - 1}):
        if dead[qi]:
            continue
        m = int(cnts[qi])
        vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[qi])), ords[qi, :m], scs[qi, :m], case.k, float(thrs[qi]), candidate_ordinals=flat,
                             referee=vo.f64_referee(sub, qs[qi]))
    eng.close()


def test_device_form_ordinal_base_and_untouched_rows():
    torch = _torch()
    case = next(c for c in mw.CASES if c.name == "nq257-rand50")
    _, store, qs = mw.case_inputs(case)
    eng, dev, bits, dev_rows, flat = _setup(case, "t256m16")
    base = 1000
    eng.set_corpus_tensor(dev, ordinal_base=base)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    out = torch.full((case.nq + 1, case.k), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_masked_wide_device(dq, bits, dev_rows, case.k, 0.0, span=mw.case_span(case), out_keys=out)
    eng.synchronize()
    host = out.cpu().numpy()
    assert (host[case.nq:] == SENTINEL).all() and not (host[: case.nq] == SENTINEL).any()
    o, s, c = _native.decode_keys(host[: case.nq])
    o2, s2, c2 = eng.search_masked_wide(qs, bits, dev_rows, case.k, 0.0, span=mw.case_span(case))
    _assert_equal_answers("device form", (o, s, c), (o2, s2, c2))
    want = eng.search_subset_batch_resident(qs, dev_rows, case.k, 0.0, remap=True)
    _assert_equal_answers("ordinal base", (o2, s2, c2), want)
    assert o2[:, 0].min() >= base
    eng.close()


def test_device_form_with_nothing_to_scan_fills_zero_keys():
    """An empty span or an empty row list: the device form writes nq x k zero keys (no tile launch), as the 32/64-query tile's device form does
    for an empty span, and leaves the rows behind them alone."""
    torch = _torch()
    case = next(c for c in mw.CASES if c.name == "mask-rand50")
    _, _, qs = mw.case_inputs(case)
    eng, dev, bits, dev_rows, flat = _setup(case, "t128")
    dq = torch.from_numpy(np.ascontiguousarray(qs[:5])).cuda()
    no_rows = torch.zeros(0, dtype=torch.int32, device="cuda")
    want = eng.search_masked_device(dq, bits, 10, 0.0, span=(5, 4))
    eng.synchronize()
    assert (want.cpu().numpy() == 0).all()
    for rows, span in ((dev_rows, (5, 4)), (no_rows, (0, case.rows - 1))):
        out = torch.full((6, 10), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        eng.search_masked_wide_device(dq, bits, rows, 10, 0.0, span=span, out_keys=out)
        eng.synchronize()
        host = out.cpu().numpy()
        assert np.array_equal(host[:5], want.cpu().numpy()) and (host[5] == SENTINEL).all(), (len(rows), span)
    eng.close()


def test_argument_errors_and_empty_shapes():
    torch = _torch()
    case = next(c for c in mw.CASES if c.name == "mask-rand50")
    v, store, qs = mw.case_inputs(case)
    eng, dev, bits, dev_rows, flat = _setup(case, "t128")
    with pytest.raises(_native.TavbError, match="k = 257"):
        eng.search_masked_wide(qs, bits, dev_rows, 257, 0.0)
    with pytest.raises(ValueError, match="outside the corpus"):
        eng.search_masked_wide(qs, bits, dev_rows, 10, 0.0, span=(0, case.rows))
    odd = torch.zeros(bits.numel() * 4 + 8, dtype=torch.uint8, device="cuda")[1:]
    lib, h = eng.lib, eng._h
    import ctypes

    q = np.ascontiguousarray(qs[:2])
    t = np.zeros(2, np.float32)
    o, s, c = np.zeros((2, 10), np.int64), np.zeros((2, 10), np.float32), np.zeros(2, np.int32)
    rc = lib.tavb_search_masked_wide(h, q.ctypes.data, 2, ctypes.c_void_p(odd.data_ptr()), case.rows, 0, case.rows - 1, ctypes.c_void_p(dev_rows.data_ptr()),
                                     len(flat), 10, t.ctypes.data, o.ctypes.data, s.ctypes.data, c.ctypes.data)
    assert rc == -1 and b"aligned" in lib.tavb_last_error()  # TAVB_E_INVALID
    assert eng.search_masked_wide(qs[:4], bits, dev_rows, 10, 0.0, span=(5, 4))[2].tolist() == [0, 0, 0, 0]  # first > last
    assert eng.search_masked_wide(qs[:0], bits, dev_rows, 10, 0.0)[0].shape == (0, 10)
    eng.close()
    eng32 = _native.Engine(0)  # an fp32 corpus: not this route's
    dev32 = torch.from_numpy(v).cuda()
    eng32.set_corpus_tensor(dev32)
    with pytest.raises(_native.TavbError, match="libtavb error -4"):  # TAVB_E_UNSUPPORTED
        eng32.search_masked_wide(qs, bits, dev_rows, 10, 0.0)
    eng32.close()


def _hits(lists):
    return [[(h.item, np.float32(h.score).view(np.uint32)) for h in hits] for hits in lists]


def test_through_the_class():
    rows, dim, nq = 1300, 64, 130
    v, _ = make_corpus(rows, dim, 7100)
    qs = make_queries(nq, dim, 7101)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype="float16")
    vb.add_embeddings(None, v)
    mask = np.random.default_rng(7102).random(rows) < 0.5
    mask[:300] = False
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.dev_bits is not None and handle.dev_rows is not None
    eng = vb.engine
    assert eng.get_option("mask_wide") == 1
    per_query = [(0.0, 0.5, 0.52, 1.5)[i % 4] for i in range(nq)]
    for k in (10, 256):
        for ms in (0.0, per_query):
            eng.set_option("mask_wide", 0)
            eng.set_option("mask_tile", 0)
            want = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=ms)
            assert eng.get_option("masked_route") == 1
            eng.set_option("mask_tile", 1)
            eng.set_option("mask_wide", 1)  # the defaults: 500 x 128 bytes are far below mask_tile_min_bytes -- the route it was
            assert _hits(vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=ms)) == _hits(want) and eng.get_option("masked_route") == 1
            eng.set_option("mask_wide", 2)
            for allowed in (handle, mask):
                got = vb.fuzzy_lookup_embeddings_masked(qs, allowed, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 3 and eng.get_option("last_tier") == 4
                assert _hits(got) == _hits(want), (k, type(allowed).__name__)
                ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs, allowed, max_hits=k, min_score=ms, as_arrays=True)
                for i, hits in enumerate(got):
                    assert cnts[i] == len(hits) and ords[i, : cnts[i]].tolist() == [h.item for h in hits] and all(mask[h.item] for h in hits)
                    if isinstance(ms, list) and ms[i] > 1:
                        assert hits == []
            # the plan followed, with its floors out of the way: 130 queries = 17 passes x 500 rows against two 128-query tiles x 1044 rows
            eng.set_option("mask_wide", 1)
            eng.set_option("mask_tile_min_bytes", 0)
            vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=ms)
            assert eng.get_option("masked_route") == 3
            vb.fuzzy_lookup_embeddings_masked(qs[:64], handle, max_hits=k, min_score=0.0)  # below mfma_min_batch: the 32/64-query tile (k <= 64) or the row list
            assert eng.get_option("masked_route") == (2 if k <= 64 else 1)
            eng.set_option("mask_tile_min_bytes", _native.MASK_TILE_MIN_BYTES)
    eng.set_option("mask_wide", 2)
    vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=300)  # beyond the route's k: the row list's large-k passes
    assert eng.get_option("masked_route") == 1


def test_fp32_corpora_and_device_groups_keep_their_routes():
    rows, dim, nq = 1300, 64, 130
    v, _ = make_corpus(rows, dim, 7200)
    qs = make_queries(nq, dim, 7201)
    mask = np.random.default_rng(7202).random(rows) < 0.5
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype="float32")
    vb.add_embeddings(None, v)
    vb.engine.set_option("mask_wide", 2)
    vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=10)
    assert vb.engine.get_option("masked_route") == 1  # (mask_tile = 1: far below its floor)
    vb.engine.set_option("mask_tile", 2)
    vb.fuzzy_lookup_embeddings_masked(qs, mask, max_hits=10)
    assert vb.engine.get_option("masked_route") == 2
    group = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 0], corpus_dtype="float16")
    group.add_embeddings(None, v)
    handle = group.row_mask(mask)
    assert handle.shards is not None and handle.dev_bits is None
    want = [group.fuzzy_lookup_embedding_in_subset(q, np.flatnonzero(mask), max_hits=10) for q in qs[:6]]
    assert _hits(group.fuzzy_lookup_embeddings_masked(qs[:6], handle, max_hits=10)) == _hits(want)
