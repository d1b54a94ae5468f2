"""GPU suite: masked batches on the 32/64-query tile -- the MASKED instantiations of `skinny_scan_kernel` behind tavb_search_masked_device
(the table is tests/masked_tile_cases.py; tests/test_masked_tile_host.py asserts the table's own claims on the CPU).

Every case forces the tile (`masked_tile_cases.ROUTE_OPTS`: the options of tests/skinny_cases.py plus `mask_tile = 2`) and runs the lookup
several ways (`masked_tile_cases.runs`): its first 32 queries (32-query tile), the whole batch (64-query tile; 65 queries: two query tiles), on
whole-line widths the 32 again under `mfma_sched` 8, 6, 5 and 9, all under every `mfma_splits` of the case.  Per case:
  1. (test_all_ones_mask_equals_the_unmasked_lookup) an all-ones mask returns the keys of `search_device` under the same options, bit for bit;
  2. all runs give identical keys in all nq x k slots: every instantiation tests the same bit for a given row;
  3. every query against the float64-refereed oracle over the allowed rows (the fp16-rounded rows of an fp16 corpus);
  4. no returned ordinal is disallowed;
  5. `masked_route` == 2, `last_tier` == 5 and `last_skinny_kernel` = the instantiation the run asked for;
  6. the output row behind the batch stays untouched and every slot of a live query is written (a sentinel fills the output first);
  7. (test_through_the_class) `fuzzy_lookup_embeddings_masked` with `mask_tile` = 2 on a handle and on a raw mask, `as_arrays` and per-query
     thresholds; with `mask_tile` = 0 and at the defaults (these corpora are far below `mask_tile_min_bytes`) the gather route runs and
     returns what the sequential subset lookups return, bit for bit.
Cases whose seed is odd hand the library a last word whose bits behind the corpus are ones: they "may hold anything".

Mutations, each built into a scratch copy of the library and run once over the 105 cases of this file:
  * `bit = (r_off ^ 1) + 4 * (lane >> 5)` in the kernel's bit test: 54 cases fail (52 of the table, both class tests).  The 16 table cases that
    pass cannot see a swap inside an even / odd pair of rows: the all-ones, empty and whole-word masks, the ranges (their ends are even), and
    the one-row corpus whose last word carries garbage; the 34 all-ones comparisons pass by construction.
  * the per-phase word offset dropped in the route (every phase reads the span's first words): the 6 ladder cases fail, nothing else has
    more than one phase.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import masked_tile_cases as mc
from tests import skinny_cases as sc
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF
GETTERS = ("masked_route", "last_tier", "last_shadow", "last_skinny_kernel")


def _torch():
    import torch

    return torch


def _engine(case: mc.Case, store: np.ndarray):
    torch = _torch()
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*mc.ROUTE_OPTS, *case.opts):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev)
    return eng, dev


def _bits(words: np.ndarray):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _masked_runs(eng, case: mc.Case, dq, bits, span, thrs, unmasked_thr=None) -> dict:
    """every run of the case -> {run: keys [run.nq, k]}; unmasked_thr: through `search_device` instead (no mask)"""
    torch = _torch()
    got = {}
    for run in mc.runs(case):
        eng.set_option("mfma_splits", run.splits)
        eng.set_option("mfma_sched", run.sched)
        out = torch.full((run.nq + 1, case.k), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        if unmasked_thr is None:
            eng.search_masked_device(dq[: run.nq], bits, case.k, thrs[: run.nq], span=span, out_keys=out)
        else:
            eng.search_device(dq[: run.nq], case.k, unmasked_thr, out_keys=out)
        eng.synchronize()
        if span[0] <= span[1]:  # (an empty span launches nothing)
            state = {g: eng.get_option(g) for g in GETTERS}
            want = {"masked_route": 2 if unmasked_thr is None else state["masked_route"], "last_tier": 5, "last_shadow": 0, "last_skinny_kernel": run.kernel}
            assert state == want, f"{case.name} {run.what}: want {want}, got {state}"
        host = out.cpu().numpy()
        assert (host[run.nq:] == SENTINEL).all(), f"{case.name} {run.what}: keys written behind the last live query"
        assert not (host[: run.nq] == SENTINEL).any(), f"{case.name} {run.what}: slots of a live query left unwritten"
        got[run] = host[: run.nq].copy()
    eng.set_option("mfma_splits", 0)
    eng.set_option("mfma_sched", 0)
    return got


def _assert_identical(case: mc.Case, got: dict) -> np.ndarray:
    full_run, full = next((r, k) for r, k in got.items() if r.nq == case.nq and r.sched == 0)
    for run, keys in got.items():
        diff = keys != full[: run.nq]
        if diff.any():
            where = np.argwhere(diff)
            o_a, _, _ = _native.decode_keys(keys)
            o_b, _, _ = _native.decode_keys(full[: run.nq])
            q0 = int(where[0][0])
            only = sorted(set(o_a[q0].tolist()) ^ set(o_b[q0].tolist()))
            raise AssertionError(f"{case.name}: run ({run.what}, kernel {run.kernel}) and run ({full_run.what}, kernel {full_run.kernel}) differ in "
                                 f"{int(diff.sum())} of {keys.size} keys; first at (query, slot) {where[:4].tolist()}; rows in one answer only {only[:12]} "
                                 f"(row mod 256: {[r % 256 for r in only[:12]]})")
    return full


@pytest.mark.parametrize("case", mc.CASES, ids=[c.name for c in mc.CASES])
def test_masked_tile_case(case):
    torch = _torch()
    v, store, qs = mc.case_inputs(case)
    mask = mc.case_mask(case)
    flat = np.flatnonzero(mask)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = _bits(mc.case_words(case, garbage=mc.case_garbage(case)))
    thrs = mc.case_thresholds(case)
    span = mc.case_span(case)
    keys = _assert_identical(case, _masked_runs(eng, case, dq, bits, (1, 0) if span is None else span, thrs))
    ords, scs, cnts = _native.decode_keys(keys)
    if len(flat) == 0:
        assert (keys == 0).all(), f"{case.name}: an empty mask returned keys"
        eng.close()
        return
    sub = v[flat]  # the reference: the allowed rows, once
    dead = np.isnan(thrs) | (thrs > 1)
    for qi in range(case.nq):
        m = int(cnts[qi])
        bad = [int(o) for o in ords[qi, :m] if not (0 <= o < case.rows and mask[o])]
        assert not bad, f"{case.name}: query {qi} returned disallowed rows {bad[:12]} (row mod 256: {[r % 256 for r in bad[:12]]}, word {[r // 32 for r in bad[:12]]})"
        if dead[qi]:
            assert m == 0, (case.name, qi)
            continue
        if thrs[qi] == 0:
            assert m == min(case.k, len(flat)), f"{case.name}: query {qi} returned {m} of {min(case.k, len(flat))} allowed rows"
        try:
            vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[qi])), ords[qi, :m], scs[qi, :m], case.k, float(thrs[qi]), candidate_ordinals=flat,
                                 referee=vo.f64_referee(sub, qs[qi]))
        except AssertionError as e:
            want = set(flat[sc.oracle_topk_rows(sub, qs[qi: qi + 1], case.k)[0]].tolist())
            missing = sorted(want - set(ords[qi, :m].tolist()))
            raise AssertionError(f"{case.name}: query {qi}: {e}; of the float64 top {case.k} among the allowed rows missing {missing[:12]} "
                                 f"(row mod 256: {[r % 256 for r in missing[:12]]}, word {[r // 32 for r in missing[:12]]})") from e
    if case.thr == "mixed":
        assert dead.any() and (cnts[thrs == 0] == min(case.k, len(flat))).all()
    eng.close()


ALL_ONES = [c for c in mc.CASES if c.group in ("rows", "width", "splits", "ladder") and c.thr == "zero"]


@pytest.mark.parametrize("case", ALL_ONES, ids=[c.name for c in ALL_ONES])
def test_all_ones_mask_equals_the_unmasked_lookup(case):
    """The case's corpus under an all-ones mask (the last word's bits behind the corpus set as well) over the whole span: every run returns the
    keys of `search_device` under the same options, bit for bit -- the same phases, row ranges, MFMA sequence and selection."""
    torch = _torch()
    v, store, qs = mc.case_inputs(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = _bits(np.full((case.rows + 31) // 32, 0xFFFFFFFF, dtype=np.uint32))
    thrs = np.zeros(case.nq, dtype=np.float32)
    masked = _masked_runs(eng, case, dq, bits, (0, case.rows - 1), thrs)
    plain = _masked_runs(eng, case, dq, bits, (0, case.rows - 1), thrs, unmasked_thr=0.0)
    for run, keys in masked.items():
        np.testing.assert_array_equal(keys, plain[run], err_msg=f"{case.name} {run.what}")
    eng.close()


def test_argument_errors_and_empty_shapes():
    torch = _torch()
    case = next(c for c in mc.CASES if c.name == "mask-fp32-d64-rand50")
    v, store, qs = mc.case_inputs(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = _bits(mc.case_words(case))
    with pytest.raises(_native.TavbError, match="1 <= k <= 64"):
        eng.search_masked_device(dq, bits, 65, 0.0)
    with pytest.raises(ValueError, match="outside the corpus"):
        eng.search_masked_device(dq, bits, 10, 0.0, span=(0, case.rows))
    out = torch.full((3, 10), SENTINEL, dtype=torch.int64, device="cuda")
    eng.search_masked_device(dq[:2], bits, 10, 0.0, span=(5, 4), out_keys=out)  # first > last: zero keys
    eng.synchronize()
    host = out.cpu().numpy()
    assert (host[:2] == 0).all() and (host[2] == SENTINEL).all()
    ords, scs, cnts = eng.search_masked_batch(qs[:4], bits, 10, 0.0, span=(5, 4))
    assert cnts.tolist() == [0, 0, 0, 0]
    ords, scs, cnts = eng.search_masked_batch(qs[:0], bits, 10, 0.0)
    assert ords.shape == (0, 10)
    # the host-synchronous form equals the device form
    o, s, c = eng.search_masked_batch(qs, bits, 10, 0.0, span=mc.case_span(case))
    keys = eng.search_masked_device(dq, bits, 10, 0.0, span=mc.case_span(case))
    eng.synchronize()
    o2, s2, c2 = _native.decode_keys(keys.cpu().numpy())
    assert np.array_equal(c, c2) and np.array_equal(o, o2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
    eng.close()
    case16 = next(c for c in mc.CASES if c.name == "mask-fp16-d64-rand50")
    eng, dev = _engine(case16, np.ascontiguousarray(mc.case_inputs(case16)[1][:, :24]))  # 48-byte rows
    with pytest.raises(_native.TavbError, match="multiple of 64 bytes"):
        eng.search_masked_batch(qs[:4, :24], _bits(mc.case_words(case16)), 10, 0.0)
    eng.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_through_the_class(dtype):
    rows, dim, nq = 1300, 64, 40
    from tests.synth import make_corpus, make_queries

    v, _ = make_corpus(rows, dim, 6100)
    qs = make_queries(nq, dim, 6101)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    vv = v.astype(np.float16).astype(np.float32) if dtype == "float16" else v
    mask = np.random.default_rng(6102).random(rows) < 0.5
    mask[:300] = False
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.dev_bits is not None and handle.span == (int(flat[0]), int(flat[-1])) and handle.count == len(flat)
    eng = vb.engine
    assert eng.get_option("mask_tile") == 1 and eng.get_option("mask_tile_min_bytes") == 128 << 20 and eng.get_option("mask_tile_pct") == 100
    per_query = [(0.0, 0.5, 0.52, 1.5)[i % 4] for i in range(nq)]
    sub = vv[flat]
    for k in (10, 64):
        for ms in (0.0, per_query):
            seq = [vb.fuzzy_lookup_embedding_in_subset(q, flat, max_hits=k, min_score=ms[i] if isinstance(ms, list) else ms) for i, q in enumerate(qs)]
            # defaults, and the tile switched off: the gather route, today's answers bit for bit
            for mode in (1, 0):
                eng.set_option("mask_tile", mode)
                got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 1
                assert [[(h.item, np.float32(h.score)) for h in hits] for hits in got] == [[(h.item, np.float32(h.score)) for h in hits] for hits in seq], (k, mode)
            eng.set_option("mask_tile", 2)
            for allowed in (handle, mask):
                got = vb.fuzzy_lookup_embeddings_masked(qs, allowed, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 2 and eng.get_option("last_tier") == 5
                ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs, allowed, max_hits=k, min_score=ms, as_arrays=True)
                for i, hits in enumerate(got):
                    thr = ms[i] if isinstance(ms, list) else ms
                    assert cnts[i] == len(hits) and ords[i, : cnts[i]].tolist() == [h.item for h in hits]
                    assert all(mask[h.item] for h in hits)
                    if thr > 1:
                        assert hits == []
                        continue
                    vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [h.item for h in hits], [h.score for h in hits], k, thr, candidate_ordinals=flat,
                                         referee=vo.f64_referee(sub, qs[i]))
                    # the sequential subset lookups: the same rows (these inputs have no near tie at rank k), scores within the project's tolerance
                    assert len(hits) == len(seq[i])
                    assert max((abs(a.score - b.score) for a, b in zip(hits, seq[i])), default=0.0) <= vo.SCORE_TOL
            eng.set_option("mask_tile", 1)
    one = vb.fuzzy_lookup_embedding_masked(qs[0], handle, max_hits=5)
    assert eng.get_option("masked_route") == 1 and [h.item for h in one] == [h.item for h in vb.fuzzy_lookup_embedding_in_subset(qs[0], flat, max_hits=5)]
