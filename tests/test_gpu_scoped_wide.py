"""GPU suite: scoped batches on the 128/256-query filter tile + exact rescoring -- the four `mfma_scan_scoped_kernel` instantiations behind
tavb_search_scoped_wide_device (the table is tests/scoped_wide_cases.py; tests/test_scoped_wide_host.py is the CPU twin).

Every case forces the route (`scoped_wide_cases.ROUTE_OPTS`) and runs on each of its variants (the 128-query tile and the three forms of the
256-query tile, forced as tests/masked_wide_cases.py forces them).  Per (case, variant):
  1. the keys EQUAL `search_scoped_device`'s (the row-list route) on the same inputs bit for bit, in all nq x k slots -- ordinals, float32
     score bits and counts; no case excluded, no near-tie allowance: the rescoring makes the route exact;
  2. `masked_route` == 6, `last_tier` == 4, `last_mfma_shape` = the variant's MFMA, `last_shadow` = the width needs the padded copy;
  3. the output row behind the batch stays untouched and every slot of a live query is written (a sentinel fills the output first);
  4. the flagged cases report `last_flagged` >= 1 (the re-run landed in the right slot, or 1. fails);
and per case, on the (equal) keys: every query against the float64-refereed oracle over ITS OWN scope under `SCORE_TOL`, no returned ordinal
outside that scope, min(k, |scope|) hits at threshold 0.
Then: one mask in nq distinct buffers equals `search_masked_wide_device` bit for bit; all-ones scopes equal the unmasked wide lookup; the
host-synchronous and the message form equal their row-list twins; the class under `scope_wide` = 2 reports route 6, equals the loop over
`fuzzy_lookup_embedding_masked` and serves max_hits = 256 in one submission; the refusals carry their messages.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import scoped_wide_cases as sw
from tests.fakes import NullModel
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789ABCDEF


def _torch():
    import torch

    return torch


def _engine(case: sw.Case, store: np.ndarray, extra=()):
    torch = _torch()
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*sw.ROUTE_OPTS, *case.opts, *extra):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev)
    return eng, dev


def _bits(words: np.ndarray):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).copy()).cuda()


def _set(eng, opts):
    for name, val in opts:
        eng.set_option(name, val)


def _reset_variant(eng):
    _set(eng, (("mfma_tile", 0), ("mfma_shape", 16), ("mfma_bdirect", 0)))


def _call(eng, nq, k, fn):
    """fn(out) enqueues a device-resident lookup of nq queries -> its keys [nq, k]; checks the sentinel row and the live slots"""
    torch = _torch()
    out = torch.full((nq + 1, k), SENTINEL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    fn(out)
    eng.synchronize()
    host = out.cpu().numpy()
    assert (host[nq:] == SENTINEL).all(), "keys written behind the last live query"
    assert not (host[:nq] == SENTINEL).any(), "slots of a live query left unwritten"
    return host[:nq].copy()


def _describe(case, variant, want, got, scopes):
    diff = np.argwhere(want != got)
    q = int(diff[0, 0])
    wo, ws, wc = _native.decode_keys(want[q: q + 1])
    go, gs, gc = _native.decode_keys(got[q: q + 1])
    missing = sorted(set(wo[0, : wc[0]].tolist()) - set(go[0, : gc[0]].tolist()))
    extra = sorted(set(go[0, : gc[0]].tolist()) - set(wo[0, : wc[0]].tolist()))
    return (f"{case.name} {variant}: {len(diff)} of {want.size} keys differ from the row-list route's, first at (query, slot) {diff[:4].tolist()}; query {q} "
            f"(bit {q % 32} of block {q // 32}, {int(scopes[q].sum())} rows in scope): counts {int(wc[0])} -> {int(gc[0])}, missing rows {missing[:12]} "
            f"(mod 320: {[r % 320 for r in missing[:12]]}), extra rows {extra[:12]}")


@pytest.mark.parametrize("case", sw.CASES, ids=[c.name for c in sw.CASES])
def test_scoped_wide_case(case):
    torch = _torch()
    v, store, qs = sw.case_inputs(case)
    scopes = sw.case_scopes(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(sw.scope_words(s, garbage=sw.case_garbage(case))) for s in scopes]
    thrs = sw.case_thresholds(case)
    span = sw.union_span(scopes)
    nq, k = case.nq, case.k
    call_span = (1, 0) if span is None else span
    want = _call(eng, nq, k, lambda out: eng.search_scoped_device(dq, bits, k, thrs, out_keys=out))
    assert eng.get_option("masked_route") == 4
    for variant in case.variants:
        _set(eng, sw.variant_opts(variant))
        got = _call(eng, nq, k, lambda out: eng.search_scoped_wide_device(dq, bits, k, thrs, span=call_span, out_keys=out))
        if span is not None:  # (an empty span launches nothing)
            state = {g: eng.get_option(g) for g in ("masked_route", "last_tier", "last_mfma_shape", "last_shadow")}
            assert state == {"masked_route": 6, "last_tier": 4, "last_mfma_shape": sw.variant_shape(variant), "last_shadow": int(case.dim % 64 != 0)}, (case.name, variant, state)
        flagged = eng.get_option("last_flagged") if span is not None else 0
        print(f"{case.name} {variant}: last_flagged {flagged}, keys differing {int((want != got).sum())}")
        if case.dups:
            assert flagged >= 1, (case.name, variant)
        assert np.array_equal(want, got), _describe(case, variant, want, got, scopes)
        _reset_variant(eng)
    ords, scs, cnts = _native.decode_keys(want)
    dead = np.isnan(thrs) | (thrs > 1)
    for qi in range(nq):
        m = int(cnts[qi])
        flat = np.flatnonzero(scopes[qi])
        bad = [int(o) for o in ords[qi, :m] if not (0 <= o < case.rows and scopes[qi][o])]
        assert not bad, f"{case.name}: query {qi} returned rows outside its scope {bad[:12]}"
        if dead[qi] or len(flat) == 0:
            assert m == 0 and (want[qi] == 0).all(), (case.name, qi)
            continue
        if thrs[qi] == 0:
            assert m == min(k, len(flat)), f"{case.name}: query {qi} returned {m} of {min(k, len(flat))} rows of its scope"
        sub = v[flat]
        vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[qi])), ords[qi, :m], scs[qi, :m], k, float(thrs[qi]), candidate_ordinals=flat,
                             referee=vo.f64_referee(sub, qs[qi]))
    eng.close()


EQUAL = [c for c in sw.CASES if c.name in ("nq257-random50%", "family-nested", "tail-r81", "k256", "thr-mixed", "ladder-random50%", "splits-random50%", "waves-random50%")]


@pytest.mark.parametrize("case", EQUAL, ids=[c.name for c in EQUAL])
def test_one_mask_in_distinct_buffers_equals_the_masked_wide_route(case):
    """nq buffers that hold the same bits: every plane word is 0 or all ones over the live queries -- the keys of `search_masked_wide_device`
    with that mask under the same options, bit for bit"""
    torch = _torch()
    v, store, qs = sw.case_inputs(case)
    mask = np.random.default_rng(case.seed + 5).random(case.rows) < 0.5
    mask[: case.first] = False
    mask[case.rows // 2] = True
    flat = np.flatnonzero(mask)
    span = (int(flat[0]), int(flat[-1]))
    eng, dev = _engine(case, store, (("mask_wide", 2), ("mask_tile", 0)))
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    words = sw.scope_words(mask, garbage=sw.case_garbage(case))
    bits = [_bits(words) for _ in range(case.nq)]
    assert len({b.data_ptr() for b in bits}) == case.nq
    rows = torch.from_numpy(flat.astype(np.int32)).cuda()
    thrs = sw.case_thresholds(case)
    for variant in case.variants:
        _set(eng, sw.variant_opts(variant))
        a = _call(eng, case.nq, case.k, lambda out: eng.search_scoped_wide_device(dq, bits, case.k, thrs, span=span, out_keys=out))
        assert eng.get_option("masked_route") == 6
        b = _call(eng, case.nq, case.k, lambda out: eng.search_masked_wide_device(dq, bits[0], rows, case.k, thrs, span=span, out_keys=out))
        assert eng.get_option("masked_route") == 3
        np.testing.assert_array_equal(a, b, err_msg=f"{case.name} {variant}")
        _reset_variant(eng)
    eng.close()


@pytest.mark.parametrize("case", EQUAL, ids=[c.name for c in EQUAL])
def test_all_ones_scopes_equal_the_unmasked_wide_lookup(case):
    """every scope all ones (the last word's bits behind the corpus set as well), each in its own buffer, over the whole corpus: the keys of
    `search_device` on the 128/256-query tile under the same options, bit for bit"""
    torch = _torch()
    v, store, qs = sw.case_inputs(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(np.full((case.rows + 31) // 32, 0xFFFFFFFF, dtype=np.uint32)) for _ in range(case.nq)]
    thr = {"zero": 0.0, "half": 0.5, "mixed": 0.52}[case.thr]  # (the unmasked device form takes one threshold for the batch)
    for variant in case.variants:
        _set(eng, sw.variant_opts(variant))
        a = _call(eng, case.nq, case.k, lambda out: eng.search_scoped_wide_device(dq, bits, case.k, thr, span=(0, case.rows - 1), out_keys=out))
        b = _call(eng, case.nq, case.k, lambda out: eng.search_device(dq, case.k, thr, out_keys=out))
        assert eng.get_option("last_tier") == 4, "the unmasked lookup did not take the 128/256-query tile"
        np.testing.assert_array_equal(a, b, err_msg=f"{case.name} {variant}")
        _reset_variant(eng)
    eng.close()


def _same_lists(o, s, o0, s0, counts) -> bool:
    """the first counts[q] ordinals and float32 score bits of every query (the slots behind a list hold nothing)"""
    live = np.arange(o.shape[1])[None, :] < np.asarray(counts)[:, None]
    return bool(np.array_equal(o[live], o0[live]) and np.array_equal(s.view(np.uint32)[live], s0.view(np.uint32)[live]))


def test_host_and_message_forms_equal_their_row_list_twins():
    torch = _torch()
    case = next(c for c in sw.CASES if c.name == "thr-mixed")
    v, store, qs = sw.case_inputs(case)
    scopes = sw.case_scopes(case)
    eng, dev = _engine(case, store)
    bits = [_bits(sw.scope_words(s)) for s in scopes]
    thrs = sw.case_thresholds(case)
    span = sw.union_span(scopes)
    eng.set_row_messages(np.random.default_rng(11).integers(-1, 90, case.rows))
    for k in (10, 256):
        o0, s0, c0 = eng.search_scoped_batch(qs, bits, k, thrs)
        m0, ms0, mc0 = eng.search_messages_scoped(qs, bits, k, thrs, k)
        for variant in ("t128", "t256m16"):
            _set(eng, sw.variant_opts(variant))
            o, s, c = eng.search_scoped_wide(qs, bits, k, thrs, span=span)
            assert eng.get_option("masked_route") == 6
            assert np.array_equal(c, c0) and _same_lists(o, s, o0, s0, c0), (k, variant)
            m, ms, mc = eng.search_messages_scoped_wide(qs, bits, k, thrs, k, span=span)
            assert eng.get_option("masked_route") == 6
            assert np.array_equal(mc, mc0) and _same_lists(m, ms, m0, ms0, mc0), (k, variant)
            _reset_variant(eng)
    eng.close()


def test_argument_errors_on_the_device():
    torch = _torch()
    case = next(c for c in sw.CASES if c.name == "k10")
    v, store, qs = sw.case_inputs(case)
    scopes = sw.case_scopes(case)
    eng, dev = _engine(case, store)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    bits = [_bits(sw.scope_words(s)) for s in scopes]
    span = sw.union_span(scopes)
    with pytest.raises(_native.TavbError, match="row-list route"):
        eng.search_scoped_wide_device(dq, bits, 257, 0.0, span=span)
    with pytest.raises(ValueError, match="k must be >= 1"):
        eng.search_scoped_wide(qs, bits, 0, 0.0, span=span)
    with pytest.raises(ValueError, match="outside the corpus"):
        eng.search_scoped_wide_device(dq, bits, 10, 0.0, span=(0, case.rows))
    with pytest.raises(ValueError, match=f"{case.nq - 1} masks for {case.nq} queries"):
        eng.search_scoped_wide(qs, bits[:-1], 10, 0.0, span=span)
    # an empty span: zero keys, zero counts, nothing launched
    out = torch.full((3, 10), SENTINEL, dtype=torch.int64, device="cuda")
    eng.search_scoped_wide_device(dq[:2], bits[:2], 10, 0.0, span=(5, 4), out_keys=out)
    eng.synchronize()
    host = out.cpu().numpy()
    assert (host[:2] == 0).all() and (host[2] == SENTINEL).all()
    assert eng.search_scoped_wide(qs[:4], bits[:4], 10, 0.0, span=(5, 4))[2].tolist() == [0, 0, 0, 0]
    eng.close()
    eng32 = _native.Engine(0)
    dev32 = torch.from_numpy(v).cuda()
    eng32.set_corpus_tensor(dev32)
    with pytest.raises(_native.TavbError, match="fp16 corpora"):
        eng32.search_scoped_wide(qs[:4], bits[:4], 10, 0.0, span=span)
    eng32.close()


def test_through_the_class():
    rows, dim, nq = 1300, 64, 150  # (the thirty queries of the empty scope take no slot: 120 are searched)
    from tests.synth import make_corpus, make_queries

    v, _ = make_corpus(rows, dim, 6400)
    qs = make_queries(nq, dim, 6401)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype="float16")
    vb.add_embeddings(None, v)
    vb.set_row_messages(np.random.default_rng(6403).integers(-1, 90, rows))
    rng = np.random.default_rng(6402)
    pool = [rng.random(rows) < p for p in (0.5, 0.5, 0.2, 0.9)] + [np.zeros(rows, dtype=bool)]
    pool[0][:300] = False
    scopes = [pool[i % len(pool)] for i in range(nq)]
    handles = {id(m): vb.row_mask(m) for m in pool}
    assert all(isinstance(h, RowMask) and h.dev_bits is not None for h in handles.values())
    as_handles = [handles[id(m)] for m in scopes]
    eng = vb.engine
    per_query = [(0.0, 0.5, 0.52, 1.5)[i % 4] for i in range(nq)]
    key = lambda lists: [[(h.item, np.float32(h.score).tobytes()) for h in hits] for hits in lists]  # noqa: E731
    for k in (10, 256):
        for ms in (0.0, per_query):
            seq = [vb.fuzzy_lookup_embedding_masked(q, as_handles[i], max_hits=k, min_score=ms[i] if isinstance(ms, list) else ms) for i, q in enumerate(qs)]
            eng.set_option("scope_wide", 0)  # today's routes: the row list (corpora this small are below the plans' floors)
            got = vb.fuzzy_lookup_embeddings_scoped(qs, as_handles, max_hits=k, min_score=ms)
            assert eng.get_option("masked_route") == 4 and key(got) == key(seq)
            msgs0 = vb.lookup_messages_by_embeddings_scoped(qs, as_handles, k, ms)
            eng.set_option("scope_wide", 2)
            for given in (as_handles, scopes):
                got = vb.fuzzy_lookup_embeddings_scoped(qs, given, max_hits=k, min_score=ms)
                assert eng.get_option("masked_route") == 6 and eng.get_option("last_tier") == 4, k
                assert key(got) == key(seq), k
                ords, scs, cnts = vb.fuzzy_lookup_embeddings_scoped(qs, given, max_hits=k, min_score=ms, as_arrays=True)
                assert all(cnts[i] == len(hits) and ords[i, : cnts[i]].tolist() == [h.item for h in hits] for i, hits in enumerate(got))
            msgs = vb.lookup_messages_by_embeddings_scoped(qs, as_handles, k, ms)
            assert eng.get_option("masked_route") == 6
            assert key(msgs) == key(msgs0)
    eng.set_option("scope_wide", 1)  # the plan: a corpus this small is below its floor
    vb.fuzzy_lookup_embeddings_scoped(qs, as_handles, max_hits=10)
    assert eng.get_option("masked_route") == 4
