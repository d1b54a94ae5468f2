"""GPU suite: the large-k selection and the sorted route (csrc/tavb_topk.hip, the ScoreSink / MessageMaxSink epilogues of
csrc/tavb_scan.hip) on planted exact scores -- every case of tests/large_k_planted_cases.py (tests/test_large_k_planted_host.py is the
CPU twin that pins the table).  One test id per FAMILY of the table: the test runs every case of its family, lets a failed assertion of one
case stop none of the others, and fails with the names and messages of all that failed (any other error -- a failed library call -- ends
the test at once).  Every row's score bits are chosen by the table, so nothing here has a tolerance: ordinals, score
bits and counts equal the numpy expectation bit for bit in every query of the batch, slots past the count of the device forms are zero,
"last_topk_refine" equals the round count of the host model of `resolve` (integer arithmetic after the bucket map), "last_tier" is the
tabled one, and the emit-all route (tavb_search_all) returns the same arrays."""

import functools
from ctypes import c_void_p

import numpy as np
import pytest

from tests import large_k_planted_cases as pc
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=6)
def _index(corpus: str) -> VectorBase:
    """one index per corpus, shared by its cases (they follow one another in the table)"""
    p = pc.corpus_of(corpus)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=p.dtype)
    vb.add_embeddings(None, pc.planted_corpus(p.cos, p.dim, p.dtype))
    eng = vb.engine
    if p.row_to_msg is not None:
        eng.set_row_messages(p.row_to_msg)
        # (the binding takes n_messages from the map's largest value; the table's may be smaller: the values beyond it name no message)
        _native._check(eng.lib, eng.lib.tavb_set_row_messages(eng._h, c_void_p(eng.row_messages.data_ptr()), len(p.row_to_msg), p.n_messages))
    return vb


def _engine(case: pc.Case):
    eng = _index(case.corpus).engine
    eng.set_option("topk_buckets", case.buckets)
    eng.set_option("topk_boundary_keys", case.cap)
    return eng


def _same(what, got_ords, got_scores, want_ords, want_bits):
    np.testing.assert_array_equal(np.asarray(got_ords, dtype=np.int64), want_ords, err_msg=f"{what}: ordinals")
    np.testing.assert_array_equal(np.ascontiguousarray(got_scores, dtype=np.float32).view(np.uint32), want_bits, err_msg=f"{what}: score bits")


def _expected_keys(case: pc.Case, k: int) -> np.ndarray:
    """uint64 [nq, k]: the packed keys of the expectation, zero past the count"""
    out = np.zeros((case.nq, k), dtype=np.uint64)
    for q in range(case.nq):
        ords, bits = pc.expected(case, q)
        out[q, : len(ords)] = (bits.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ords.astype(np.uint64))
    return out


def _device_queries(eng, qs):
    import torch

    return torch.from_numpy(qs).to(torch.device("cuda", eng.device))


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_planted_family(family):
    cases = [c for c in pc.CASES if c.family == family]
    assert cases
    failed = []
    for case in cases:
        try:
            check_planted_case(case)
        except AssertionError as e:
            failed.append(f"[{case.name}] {e}")
    assert not failed, f"{len(failed)} of {len(cases)} cases of family {family} failed:\n" + "\n".join(failed)


def check_planted_case(case):
    import torch

    eng = _engine(case)
    p = pc.corpus_of(case.corpus)
    qs = pc.queries(case)
    thr = np.asarray(case.thr, dtype=np.float32)
    want = [pc.expected(case, q) for q in range(case.nq)]
    if case.call == "sorted":
        ords, scs, cnts = eng.search_sorted(qs, case.k, thr)
        assert cnts.tolist() == [len(w[0]) for w in want], case.name
        off = 0
        for q, (wo, wb) in enumerate(want):
            _same(f"{case.name} q{q}", ords[off : off + len(wo)], scs[off : off + len(wo)], wo, wb)
            off += len(wo)
        assert off == len(ords)
    else:
        dev_rows = eng.rows_to_device(p.row_list) if p.row_list is not None else None
        if case.call == "topk":
            ords, scs, cnts = eng.search_topk(qs, case.k, thr)
        else:
            ords, scs, cnts = eng.search_top_messages(qs, case.k, thr, dev_rows=dev_rows)
        assert cnts.tolist() == [len(w[0]) for w in want], case.name
        for q, (wo, wb) in enumerate(want):
            _same(f"{case.name} q{q}", ords[q, : cnts[q]], scs[q, : cnts[q]], wo, wb)
    assert eng.get_option("last_topk_refine") == pc.expected_rounds(case), f"{case.name}: rounds per query {[pc.model(case, q).rounds for q in range(case.nq)]}"
    assert eng.get_option("last_tier") == case.tier
    if case.call != "sorted":
        # the device form: all nq x k keys, zero past the count, and the rounds reported at the synchronise
        dq = _device_queries(eng, qs)
        torch.cuda.synchronize()
        if case.call == "topk":
            keys = eng.search_topk_device(dq, case.k, thr)
        else:
            keys = eng.search_top_messages_device(dq, case.k, thr, dev_rows=dev_rows)
        eng.synchronize()
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), _expected_keys(case, case.k), err_msg=f"{case.name}: device keys")
        assert eng.get_option("last_topk_refine") == pc.expected_rounds(case)
    if case.call != "messages":
        # the emit-all route (what "large_k" = 0 / "sort_all" = 0 send the class through) over the same per-row arithmetic
        for q, (wo, wb) in enumerate(want):
            eo, es = eng.search_all(qs[q], thr[q], None if case.k == 0 else case.k)
            _same(f"{case.name} q{q} emit-all", eo, es, wo, wb)


def test_through_the_class():
    """A case that fits, one that refines and a sorted one through VectorBase.fuzzy_lookup_embedding(s), with the device routes on and off."""
    by = {c.name: c for c in pc.CASES}
    for name in pc.CLASS_CASES:
        case = by[name]
        vb = _index(case.corpus)
        eng = _engine(case)
        q = pc.queries(case)[0]
        wo, wb = pc.expected(case, 0)
        for on in (1, 0):
            eng.set_option("large_k", on)
            eng.set_option("sort_all", on)
            res = vb.fuzzy_lookup_embedding(q, max_hits=case.k, min_score=case.thr[0])
            _same(f"{name} single on={on}", [r.item for r in res], [r.score for r in res], wo, wb)
            batch = vb.fuzzy_lookup_embeddings(np.stack([q, q]), max_hits=case.k, min_score=case.thr[0])
            for res in batch:
                _same(f"{name} batch on={on}", [r.item for r in res], [r.score for r in res], wo, wb)
            if on and case.call == "topk":
                assert eng.get_option("last_topk_refine") == pc.expected_rounds(case)
        eng.set_option("large_k", 1)
        eng.set_option("sort_all", 1)
