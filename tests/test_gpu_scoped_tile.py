"""GPU suite: scoped batches on the 32/64-query tile -- the SCOPED instantiations of `skinny_scan_kernel` and `scope_planes_kernel` behind
tavb_search_scoped_tile_device (the table is tests/scoped_tile_cases.py; tests/test_scoped_tile_host.py is the CPU twin).

Every case forces the tile (`scoped_tile_cases.ROUTE_OPTS`: the options of tests/skinny_cases.py plus `scope_tile = 2`) and runs the lookup
several ways (`scoped_tile_cases.runs`): its first 32 queries (32-query tile), the whole batch (64-query tiles), on whole-line widths the 32
again under `mfma_sched` 8, 6, 5 and 9, all under every `mfma_splits` of the case.  Per case:
  1. `tavb_scope_planes` equals the numpy planes word for word (odd seeds: the masks' last words carry ones behind the corpus);
  2. all runs give identical keys in all nq x k slots;
  3. every query against the float64-refereed oracle over ITS OWN scope (the fp16-rounded rows of an fp16 corpus), no returned ordinal
     outside that scope, min(k, |scope|) hits at threshold 0;
  4. (test_one_mask_in_distinct_buffers...) nq distinct buffers holding one mask return `search_masked_device`'s keys bit for bit;
  5. (test_all_ones_scopes...) all-ones scopes return `search_device`'s keys bit for bit;
  6. `masked_route` == 5, `last_tier` == 5 and `last_skinny_kernel` = the instantiation the run asked for;
  7. the output row behind the batch stays untouched and every slot of a live query is written (a sentinel fills the output first);
  8. (test_through_the_class) handles and raw arrays, `as_arrays`, per-query thresholds, the message form, and today's route 4 with its
     answers bit for bit at the defaults and under `scope_tile` = 0;
  9. (test_argument_errors_on_the_device) every refusal with its message.

Mutations, each built into a scratch copy of the library and run once over the 169 tests of this file (118 table cases, 24 + 24 equality
cases, the argument test, two class tests):
  * the low and the high half of a row pair's lane mask swapped (`plane[r + 4] | plane[r] << 32`): 147 tests fail -- 101 table cases, all 24
    one-mask comparisons, 20 of the 24 all-ones comparisons (the four that pass have no row r <= last < r + 4 where the halves differ) and
    both class tests.  The 17 table cases that pass cannot see the swap: all seven all_empty cases, and ten whose non-empty scopes are
    all rows (one_empty, all_rows, a single disjoint query: rows r and r + 4 lie in the same scopes) or next to nothing (random1% over 1 and 33 rows).
  * the plane of block `ni ^ 1` taken in the 64-query tile: 104 tests fail -- 70 table cases and 17 + 17 equality cases.  All 48 table cases
    and the 7 + 7 equality cases that pass run batches of up to 32 queries only (the 32-query tile has one block) or have only empty scopes.  The
    class tests passed: with 40 queries they searched 32 (the empty scopes take no slot), one block.  They run 45 queries since (36
    searched: a 64-query tile with four queries in its second block); that form was not run under the mutation.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_tile_cases as st
from tests import skinny_cases as sc
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF
GETTERS = ("masked_route", "last_tier", "last_shadow", "last_skinny_kernel")


def _torch():
    import torch

    return torch


def _engine(case: st.Case, store: np.ndarray):
    torch = _torch()
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*st.ROUTE_OPTS, *case.opts):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev)
    return eng, dev


def _bits(words: np.ndarray):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _runs(eng, case: st.Case, dq, call) -> dict:
    """every run of the case -> {run: keys [run.nq, k]}; call(nq, out) enqueues the lookup of the first nq queries; returns the route it must report"""
    torch = _torch()
    got = {}
    for run in st.runs(case):
        eng.set_option("mfma_splits", run.splits)
        eng.set_option("mfma_sched", run.sched)
        out = torch.full((run.nq + 1, case.k), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        route = call(run.nq, out)
        eng.synchronize()
        if route is not None:
            state = {g: eng.get_option(g) for g in GETTERS}
            want = {"masked_route": state["masked_route"] if route < 0 else route, "last_tier": 5, "last_shadow": 0, "last_skinny_kernel": run.kernel}
            assert state == want, f"{case.name} {run.what}: want {want}, got {state}"
        host = out.cpu().numpy()
        assert (host[run.nq:] == SENTINEL).all(), f"{case.name} {run.what}: keys written behind the last live query"
        assert not (host[: run.nq] == SENTINEL).any(), f"{case.name} {run.what}: slots of a live query left unwritten"
        got[run] = host[: run.nq].copy()
    eng.set_option("mfma_splits", 0)
    eng.set_option("mfma_sched", 0)
    return got


def _assert_identical(case: st.Case, got: dict) -> np.ndarray:
    full_run, full = next((r, k) for r, k in got.items() if r.nq == case.nq and r.sched == 0)
    for run, keys in got.items():
        diff = keys != full[: run.nq]
        if diff.any():
            where = np.argwhere(diff)
            raise AssertionError(f"{case.name}: run ({run.what}, kernel {run.kernel}) and run ({full_run.what}, kernel {full_run.kernel}) differ in "
                                 f"{int(diff.sum())} of {keys.size} keys; first at (query, slot) {where[:4].tolist()}")
    return full


@pytest.mark.parametrize("case", st.CASES, ids=[c.name for c in st.CASES])
def test_scoped_tile_case(case):
    torch = _torch()
    v, store, qs = st.case_inputs(case)
    scopes = st.case_scopes(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(st.scope_words(s, garbage=st.case_garbage(case))) for s in scopes]
    thrs = st.case_thresholds(case)
    span = st.union_span(scopes)
    if span is not None:  # 1. the planes, of the whole batch and of its first 32 queries
        for n in sorted({min(32, case.nq), case.nq}):
            planes = eng.scope_planes(bits[:n], span=span)
            eng.synchronize()
            np.testing.assert_array_equal(planes.cpu().numpy().view(np.uint32), st.planes_numpy(scopes[:n], *span), err_msg=f"{case.name}: planes of {n} scopes")

    def call(nq, out):
        eng.search_scoped_tile_device(dq[:nq], bits[:nq], case.k, thrs[:nq], span=(1, 0) if span is None else span, out_keys=out)
        return None if span is None else 5  # (an empty span launches nothing)

    keys = _assert_identical(case, _runs(eng, case, dq, call))
    ords, scs, cnts = _native.decode_keys(keys)
    dead = np.isnan(thrs) | (thrs > 1)
    for qi in range(case.nq):
        m = int(cnts[qi])
        flat = np.flatnonzero(scopes[qi])
        bad = [int(o) for o in ords[qi, :m] if not (0 <= o < case.rows and scopes[qi][o])]
        assert not bad, f"{case.name}: query {qi} returned rows outside its scope {bad[:12]} (row mod 256: {[r % 256 for r in bad[:12]]})"
        if dead[qi] or len(flat) == 0:
            assert m == 0 and (keys[qi] == 0).all(), (case.name, qi)
            continue
        if thrs[qi] == 0:
            assert m == min(case.k, len(flat)), f"{case.name}: query {qi} returned {m} of {min(case.k, len(flat))} rows of its scope"
        sub = v[flat]
        try:
            vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[qi])), ords[qi, :m], scs[qi, :m], case.k, float(thrs[qi]), candidate_ordinals=flat,
                                 referee=vo.f64_referee(sub, qs[qi]))
        except AssertionError as e:
            want = set(flat[sc.oracle_topk_rows(sub, qs[qi: qi + 1], case.k)[0]].tolist())
            missing = sorted(want - set(ords[qi, :m].tolist()))
            raise AssertionError(f"{case.name}: query {qi} (lane {qi % 32} of block {qi // 32}): {e}; of the float64 top {case.k} of its scope missing "
                                 f"{missing[:12]} (row mod 256: {[r % 256 for r in missing[:12]]})") from e
    eng.close()


EQUAL = [c for i, c in enumerate(c for c in st.CASES if c.group == "rows") if i % 3 == 0] + [c for c in st.CASES if c.group in ("wide", "ladder", "splits")]


@pytest.mark.parametrize("case", EQUAL, ids=[c.name for c in EQUAL])
def test_one_mask_in_distinct_buffers_equals_the_masked_tile(case):
    """nq buffers that hold the same mask: every plane word is 0 or all ones over the live queries, the span is the mask's -- the keys of
    `search_masked_device` with that mask under the same options, bit for bit."""
    torch = _torch()
    v, store, qs = st.case_inputs(case)
    mask = np.random.default_rng(case.seed + 5).random(case.rows) < 0.5
    mask[case.rows // 2] = True
    flat = np.flatnonzero(mask)
    span = (int(flat[0]), int(flat[-1]))
    eng, dev = _engine(case, store)
    eng.set_option("mask_tile", 2)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    words = st.scope_words(mask, garbage=st.case_garbage(case))
    bits = [_bits(words) for _ in range(case.nq)]
    assert len({b.data_ptr() for b in bits}) == case.nq
    thrs = st.case_thresholds(case)

    def scoped(nq, out):
        eng.search_scoped_tile_device(dq[:nq], bits[:nq], case.k, thrs[:nq], span=span, out_keys=out)
        return 5

    def masked(nq, out):
        eng.search_masked_device(dq[:nq], bits[0], case.k, thrs[:nq], span=span, out_keys=out)
        return 2

    a, b = _runs(eng, case, dq, scoped), _runs(eng, case, dq, masked)
    for run, keys in a.items():
        np.testing.assert_array_equal(keys, b[run], err_msg=f"{case.name} {run.what}")
    eng.close()


@pytest.mark.parametrize("case", EQUAL, ids=[c.name for c in EQUAL])
def test_all_ones_scopes_equal_the_unmasked_lookup(case):
    """every scope all ones (the last word's bits behind the corpus set as well), each in its own buffer, over the whole span: the keys of
    `search_device` under the same options, bit for bit -- the same phases, row ranges, MFMA sequence and selection"""
    torch = _torch()
    v, store, qs = st.case_inputs(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(np.full((case.rows + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)) for _ in range(case.nq)]
    thrs = np.zeros(case.nq, dtype=np.float32)

    def scoped(nq, out):
        eng.search_scoped_tile_device(dq[:nq], bits[:nq], case.k, thrs[:nq], span=(0, case.rows - 1), out_keys=out)
        return 5

    def plain(nq, out):
        eng.search_device(dq[:nq], case.k, 0.0, out_keys=out)
        return -1

    a, b = _runs(eng, case, dq, scoped), _runs(eng, case, dq, plain)
    for run, keys in a.items():
        np.testing.assert_array_equal(keys, b[run], err_msg=f"{case.name} {run.what}")
    eng.close()


def test_argument_errors_on_the_device():
    torch = _torch()
    case = next(c for c in st.CASES if c.group == "rows" and c.dtype == "fp32" and c.rows == 1300)
    v, store, qs = st.case_inputs(case)
    scopes = st.case_scopes(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(st.scope_words(s)) for s in scopes]
    nq, span = case.nq, st.union_span(scopes)
    with pytest.raises(_native.TavbError, match="1 <= k <= 64"):
        eng.search_scoped_tile_device(dq, bits, 65, 0.0, span=span)
    with pytest.raises(ValueError, match="k must be >= 1"):
        eng.search_scoped_tile(qs, bits, 0, 0.0, span=span)
    with pytest.raises(ValueError, match="outside the corpus"):
        eng.search_scoped_tile_device(dq, bits, 10, 0.0, span=(0, case.rows))
    with pytest.raises(ValueError, match="outside the corpus"):
        eng.scope_planes(bits, span=(-1, 5))
    with pytest.raises(ValueError, match=f"{nq - 1} masks for {nq} queries"):
        eng.search_scoped_tile(qs, bits[:-1], 10, 0.0, span=span)
    lib, a = eng.lib, _native._addr
    thr = np.zeros(nq, dtype=np.float32)
    ords, scs, cnts = np.zeros((nq, 10), np.int64), np.zeros((nq, 10), np.float32), np.zeros(nq, np.int32)
    import ctypes

    ptrs = (ctypes.c_void_p * nq)(*[b.data_ptr() for b in bits])
    holed = (ctypes.c_void_p * nq)(*[None if i == 3 else b.data_ptr() for i, b in enumerate(bits)])
    for masks, rows, out, text in ((None, case.rows, a(ords), b"null dev_masks"), (holed, case.rows, a(ords), b"the mask of query 3 is null"),
                                   (ptrs, case.rows + 1, a(ords), b"the mask covers"), (ptrs, case.rows, None, b"null argument")):
        rc = lib.tavb_search_scoped_tile(eng._h, a(qs), nq, masks, rows, span[0], span[1], 10, a(thr), out, a(scs), a(cnts))
        assert rc < 0 and text in lib.tavb_last_error(), (text, lib.tavb_last_error())
    rc = lib.tavb_scope_planes(eng._h, holed, nq, case.rows, span[0], span[1], ctypes.c_void_p(bits[0].data_ptr()))
    assert rc < 0 and b"mask 3 is null" in lib.tavb_last_error()
    # an empty span: zero keys, zero counts, nothing launched
    out = torch.full((3, 10), SENTINEL, dtype=torch.int64, device="cuda")
    eng.search_scoped_tile_device(dq[:2], bits[:2], 10, 0.0, span=(5, 4), out_keys=out)
    eng.synchronize()
    host = out.cpu().numpy()
    assert (host[:2] == 0).all() and (host[2] == SENTINEL).all()
    assert eng.search_scoped_tile(qs[:4], bits[:4], 10, 0.0, span=(5, 4))[2].tolist() == [0, 0, 0, 0]
    assert eng.search_scoped_tile(qs[:0], [], 10, 0.0)[0].shape == (0, 10)
    # the host-synchronous form equals the device form
    o, s, c = eng.search_scoped_tile(qs, bits, 10, 0.0, span=span)
    keys = eng.search_scoped_tile_device(dq, bits, 10, 0.0, span=span)
    eng.synchronize()
    o2, s2, c2 = _native.decode_keys(keys.cpu().numpy())
    assert np.array_equal(c, c2) and np.array_equal(o, o2) and np.array_equal(s.view(np.uint32), s2.view(np.uint32))
    eng.close()
    eng, dev = _engine(case, np.ascontiguousarray(store[:, :12]))  # 48-byte rows
    with pytest.raises(_native.TavbError, match="multiple of 64 bytes"):
        eng.search_scoped_tile(qs[:4, :12], bits[:4], 10, 0.0, span=span)
    eng.close()


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_through_the_class(dtype):
    rows, dim, nq = 1300, 64, 45  # (the nine queries of the empty scope take no slot: 36 are searched, a 64-query tile)
    from tests.synth import make_corpus, make_queries

    v, _ = make_corpus(rows, dim, 6300)
    qs = make_queries(nq, dim, 6301)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
    vb.add_embeddings(None, v)
    rm = np.random.default_rng(6303).integers(-1, 90, rows)
    vb.set_row_messages(rm)
    vv = v.astype(np.float16).astype(np.float32) if dtype == "float16" else v
    rng = np.random.default_rng(6302)
    pool = [rng.random(rows) < p for p in (0.5, 0.5, 0.2, 0.9)] + [np.zeros(rows, dtype=bool)]
    pool[0][:300] = False
    scopes = [pool[i % len(pool)] for i in range(nq)]
    handles = {id(m): vb.row_mask(m) for m in pool}
    assert all(isinstance(h, RowMask) and h.dev_bits is not None for h in handles.values())
    eng = vb.engine
    assert eng.get_option("scope_tile") == 1
    per_query = [(0.0, 0.5, 0.52, 1.5)[i % 4] for i in range(nq)]
    for k in (10, 64):
        for ms in (0.0, per_query):
            as_handles = [handles[id(m)] for m in scopes]
            # defaults, and the tile switched off: the row-list route, today's answers bit for bit
            seq = [vb.fuzzy_lookup_embedding_masked(q, as_handles[i], max_hits=k, min_score=ms[i] if isinstance(ms, list) else ms) for i, q in enumerate(qs)]
            for mode in (1, 0):
                eng.set_option("scope_tile", mode)
                got = vb.fuzzy_lookup_embeddings_scoped(qs, as_handles, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 4
                assert [[(h.item, np.float32(h.score)) for h in hits] for hits in got] == [[(h.item, np.float32(h.score)) for h in hits] for hits in seq], (k, mode)
            msgs0 = vb.lookup_messages_by_embeddings_scoped(qs, as_handles, k, ms)
            assert eng.get_option("masked_route") == 4
            eng.set_option("scope_tile", 2)
            for given in (as_handles, scopes):
                got = vb.fuzzy_lookup_embeddings_scoped(qs, given, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 5 and eng.get_option("last_tier") == 5
                ords, scs, cnts = vb.fuzzy_lookup_embeddings_scoped(qs, given, max_hits=k, min_score=ms, as_arrays=True)
                for i, hits in enumerate(got):
                    thr = ms[i] if isinstance(ms, list) else ms
                    flat = np.flatnonzero(scopes[i])
                    assert cnts[i] == len(hits) and ords[i, : cnts[i]].tolist() == [h.item for h in hits]
                    assert all(scopes[i][h.item] for h in hits)
                    if thr > 1 or len(flat) == 0:
                        assert hits == []
                        continue
                    sub = vv[flat]
                    vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [h.item for h in hits], [h.score for h in hits], k, thr, candidate_ordinals=flat,
                                         referee=vo.f64_referee(sub, qs[i]))
                    assert len(hits) == len(seq[i])
                    assert max((abs(a.score - b.score) for a, b in zip(hits, seq[i])), default=0.0) <= vo.SCORE_TOL
            # the message form against the row-list route's: the same messages (these inputs have no near tie at a cut), scores within tolerance
            msgs = vb.lookup_messages_by_embeddings_scoped(qs, as_handles, k, ms)
            assert eng.get_option("masked_route") == 5
            for i in range(nq):
                assert [h.item for h in msgs[i]] == [h.item for h in msgs0[i]], (k, i)
                assert max((abs(a.score - b.score) for a, b in zip(msgs[i], msgs0[i])), default=0.0) <= vo.SCORE_TOL
            eng.set_option("scope_tile", 1)
