"""CPU suite of the near-duplicate self-join (`VectorBase.similarity_join`, tavb_join_pairs, tavb_plan_pairs_join), no GPU:

  * `similarity_join` on a host-only index (tests/fake_engine.py: the row lookups, which are the definition) equals
    tests/lookup_rows_cases.definition_pairs exactly and a float64 brute force outside near-ties, with and without `among`, for
    max_per_row None, 1 and 16;
  * the host sort and the per-row cut on hand-made (i, j, score) input, ties and runs longer than max_per_row included;
  * the entry points are declared, bound and exported, refuse bad arguments, and their options are documented;
  * the truth table of tavb_plan_pairs_join;
  * the numpy twin of the join's bound on every case corpus: the largest |float64 score of the fp16-rounded rows - float64 score of the
    stored rows| over all pairs lies below delta."""

import ctypes
import os

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import lookup_rows_cases as lc
from tests import pairs_join_cases as pc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_index(monkeypatch, v: np.ndarray, dtype: str = "fp32") -> VectorBase:
    monkeypatch.setattr(_native, "Engine", FakeEngine)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    vb.add_embeddings(None, np.array(v))
    return vb


@pytest.mark.parametrize("with_among", (False, True))
def test_similarity_join_on_a_host_only_index_is_the_definition(monkeypatch, with_among):
    v = pc.corpus("fp32", 400, 64)
    vb = host_index(monkeypatch, v)
    allowed = lc.among_mask(len(v)) if with_among else None

    def lookup_all(i):
        hits = vb.fuzzy_lookup_embedding(v[i], max_hits=0, min_score=pc.MIN_SCORE)
        return [h.item for h in hits], [h.score for h in hits]

    for max_per_row in (None, 1, 16):
        i, j, s = vb.similarity_join(pc.MIN_SCORE, allowed, max_per_row)
        want = lc.definition_pairs(lookup_all, len(v), pc.MIN_SCORE, max_per_row if max_per_row else len(v), allowed)
        assert list(zip(i.tolist(), j.tolist(), s.tolist())) == [(a, b, float(np.float32(c))) for a, b, c in want]
        assert (i < j).all() and s.dtype == np.float32
    # every pair, against float64: all sure pairs present, nothing reported that is clearly below the threshold
    i, j, s = vb.similarity_join(pc.MIN_SCORE, allowed)
    bi, bj, bs, full = pc.brute_pairs(v, pc.MIN_SCORE, allowed)
    got = set(zip(i.tolist(), j.tolist()))
    sure = {(a, b) for a, b, c in zip(bi.tolist(), bj.tolist(), bs.tolist()) if c >= pc.MIN_SCORE + 4 * vo.TIE_EPS}
    assert sure <= got and len(sure) >= (25 if with_among else 80)  # (100 planted pairs; a mask of 60 % keeps about a third of them)
    assert all(full[a, b] >= pc.MIN_SCORE - 4 * vo.TIE_EPS and abs(full[a, b] - c) <= vo.SCORE_TOL for a, b, c in zip(i.tolist(), j.tolist(), s.tolist()))
    if with_among:
        assert allowed[i].all() and allowed[j].all()
    with pytest.raises(ValueError):
        vb.similarity_join(0.9, None, 0)


def test_host_sort_and_per_row_cut():
    f = np.float32
    i = np.array([5, 2, 2, 2, 5, 2, 9, 2], np.int64)
    j = np.array([7, 9, 4, 8, 6, 3, 11, 6], np.int64)
    s = np.array([0.5, 0.9, 0.9, 1.0, 0.5, 0.8, 0.7, 0.9], f)
    oi, oj, os_ = VectorBase._order_pairs(i, j, s, None)
    assert list(zip(oi.tolist(), oj.tolist(), os_.tolist())) == [
        (2, 8, 1.0), (2, 4, f(0.9)), (2, 6, f(0.9)), (2, 9, f(0.9)), (2, 3, f(0.8)), (5, 6, 0.5), (5, 7, 0.5), (9, 11, f(0.7))]
    oi, oj, os_ = VectorBase._order_pairs(i, j, s, 2)  # the run of row 2 is five long; the cut falls inside a tie: ascending j decides
    assert list(zip(oi.tolist(), oj.tolist())) == [(2, 8), (2, 4), (5, 6), (5, 7), (9, 11)]
    oi, oj, os_ = VectorBase._order_pairs(i, j, s, 1)
    assert list(zip(oi.tolist(), oj.tolist())) == [(2, 8), (5, 6), (9, 11)]
    assert oi.dtype == np.int64 and oj.dtype == np.int64 and os_.dtype == f
    e = VectorBase._order_pairs(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, f), 3)
    assert all(len(x) == 0 for x in e)
    # the cut is per ROW, not per run of equal neighbours: row 0 behind row 1 never happens after the sort
    oi, oj, _ = VectorBase._order_pairs(np.array([1, 0, 1, 0]), np.array([2, 3, 3, 1]), np.array([0.6, 0.6, 0.7, 0.9], f), 1)
    assert list(zip(oi.tolist(), oj.tolist())) == [(0, 1), (1, 3)]


def test_entry_points_are_declared_bound_exported_and_refuse_bad_arguments():
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    lib = _native.load_library(preload_torch=False)
    for name in ("tavb_join_pairs", "tavb_plan_pairs_join"):
        assert f"int {name}(" in text and name in _native.ABI_SYMBOLS and hasattr(lib, name), name
    for name in ("pairs_join", "pairs_join_min_rows", "pairs_join_capacity", "pairs_join_max_capacity", "pairs_join_launches", "pairs_join_candidates"):
        assert f'"{name}"' in text, name
    assert "#define TAVB_PAIRS_NO_FIT 1" in text and "#define TAVB_PAIRS_REFUSED 2" in text
    assert (_native.PAIRS_NO_FIT, _native.PAIRS_REFUSED) == (1, 2)
    total, needed = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.tavb_join_pairs(None, ctypes.c_float(0.9), None, 8, None, None, None, ctypes.byref(total), ctypes.byref(needed))
    assert rc == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_plan_pairs_join(100, 64, 7, 1, 1, 1) == -1 and b"dtype" in lib.tavb_last_error()
    assert lib.tavb_plan_pairs_join(-1, 64, _native.TAVB_F16, 1, 1, 1) == -1
    assert lib.tavb_plan_pairs_join(100, 64, _native.TAVB_F16, 1, 1, 0) == -1
    with pytest.raises(ValueError):
        _native.plan_pairs_join(-1, 64, _native.TAVB_F16)
    # the provisional default keeps tests/test_gpu_lookup_rows.py (2000 rows) on the route it was written for
    assert _native.PAIRS_JOIN_MIN_ROWS > 2000
    src = open(os.path.join(ROOT, "typeagent_py_amd", "csrc", "tavb_ctx.h")).read()
    assert f"kPairsJoinMinRows = {_native.PAIRS_JOIN_MIN_ROWS};" in src


def test_plan_truth_table():
    F16, F32 = _native.TAVB_F16, _native.TAVB_F32
    plan = _native.plan_pairs_join
    assert plan(10_000, 1536, F16) and plan(10_000, 1536, F32) and plan(8192, 64, F16)
    assert not plan(8191, 64, F16)                       # below "pairs_join_min_rows"
    assert plan(2, 64, F16, min_rows=1) and not plan(1, 64, F16, min_rows=1) and not plan(0, 64, F16, min_rows=1)
    for dim in (72, 100, 32, 16448, 0):                   # the width rule: whole K steps of 64, at most 16384
        assert not plan(10_000, dim, F16), dim
    assert plan(10_000, 16384, F16)
    assert not plan(10_000, 64, F16, single_gpu=False)    # device groups, row shards
    assert not plan(10_000, 64, F32, has_shadow=False) and plan(10_000, 64, F16, has_shadow=False)
    assert not plan((1 << 31) - 1, 64, F16) and plan((1 << 31) - 2, 64, F16)


CASE_CORPORA = [(d, r, w) for d, r, w in pc.CORPORA] + [(d, n, 64) for n in pc.EDGE_ROWS if n > 1 for d in ("fp16", "fp32")]


def test_delta_twin_bounds_the_rounding_of_every_case_corpus():
    worst = 0.0
    for dtype, rows, dim in CASE_CORPORA:
        v = pc.stored(pc.corpus(dtype, rows, dim), dtype) if (dtype, rows, dim) in pc.CORPORA else pc.edge_corpus(rows, dim, dtype)
        delta = pc.join_delta(v, dtype, dim)
        assert np.isfinite(delta) and 1.2e-7 < delta < 2e-3, (dtype, rows, dim, delta)
        x = v.astype(np.float64)
        x16 = v.astype(np.float16).astype(np.float64)
        exact = np.clip((x @ x.T + 1.0) / 2.0, 0.0, 1.0)
        approx = np.clip((x16 @ x16.T + 1.0) / 2.0, 0.0, 1.0)
        err = np.abs(exact - approx)[np.triu_indices(len(v), 1)].max() if len(v) > 1 else 0.0
        assert err < delta, (dtype, rows, dim, err, delta)
        if dtype == "fp16":
            assert err == 0.0  # the rows ARE the fp16 values: only the summation slack is left
        worst = max(worst, err / float(delta))
        thr = pc.join_threshold(np.float32(pc.MIN_SCORE), delta)
        assert thr < np.float32(pc.MIN_SCORE) - delta
    assert 0.0 < worst < 1.0
    assert pc.join_threshold(np.float32(0.0), np.float32(1e-4)) == -np.inf
    bad = np.array(pc.corpus("fp32", 300, 64))
    bad[3, 3] = np.inf
    with np.errstate(all="ignore"):
        assert pc.join_delta(bad, "fp32", 64) == np.inf
