"""CPU twin of tests/test_gpu_query_edges.py: the table of tests/query_edge_cases.py has a well-defined oracle answer in every case, the
checker accepts that answer, and the cases have teeth -- a numpy model of the split planes (hi = float16(q), lo = float16(q - hi) or 0 where
hi is not finite, float32 accumulation) is rejected where a finite element rounds to an fp16 infinity and accepted everywhere else, and the
filter's operand alone (float16(q)) is rejected when it leaks into an answer.  No GPU."""

from __future__ import annotations

import numpy as np
import pytest

from tests import query_edge_cases as qc

CASES = qc.host_cases()


def _inputs(c: qc.HostCase):
    v, _ = qc.corpus(c.ckind, c.dim, c.dtype)
    return v, qc.make_query(c.kind, c.ckind, c.dim, c.dtype, k=c.k)


def _rejected(v, q, scores, c: qc.HostCase) -> bool:
    items, scs = qc.answer(scores, c.k, c.thr)
    try:
        qc.check_answer(v, q, items, scs, c.k, c.thr, qc.is_exact(v, q), c.name)
    except AssertionError:
        return True
    return False


def test_every_branch_has_a_case():
    have = {c.branch for c in CASES}
    assert have == set(qc.BRANCH.values())
    assert {c.kind for c in CASES} == set(qc.BRANCH)
    assert {c.k for c in CASES} >= set(qc.KS) | {0}
    for dtype, dims in qc.DIMS.items():
        for dim in dims:
            assert {c.kind for c in CASES if (c.dim, c.dtype) == (dim, dtype)} == set(qc.BRANCH)


def test_corpora_are_what_the_table_says():
    for dtype, dims in qc.DIMS.items():
        for dim in dims:
            g, _ = qc.corpus("gauss", dim, dtype)
            z, _ = qc.corpus("gauss-z", dim, dtype)
            a, b = qc.ZCOLS
            assert not (g[:, [a, b]] == 0).any()
            assert np.flatnonzero(z[:, a] > 0).tolist() == list(qc.POS_ROWS)
            assert np.flatnonzero(z[:, a] == 0).tolist() == sorted(qc.Z_A + qc.Z_AB)
            assert np.flatnonzero(z[:, b] == 0).tolist() == sorted(qc.Z_B + qc.Z_AB)
            keep = np.ones(dim, dtype=bool)
            keep[[a, b]] = False
            assert (z[:, keep] == g[:, keep]).all()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_is_well_defined_and_accepted(case):
    v, q = _inputs(case)
    s = qc.oracle_scores(v, q)
    nan_rows = np.flatnonzero(np.isnan(s))
    assert nan_rows.tolist() == qc.predicted_nan_rows(case.kind, case.ckind, case.dim, case.dtype).tolist()
    ok = s[~np.isnan(s)]
    assert ((ok >= 0) & (ok <= 1)).all()
    if case.kind in ("zero", "f32-subnormal"):
        assert (s == np.float32(0.5)).all()
    if case.kind == "nan-one":
        assert qc.answer(s, case.k, case.thr)[0].size == 0
    if case.kind in qc.NONFINITE_KINDS:
        assert set(np.unique(ok).tolist()) <= {0.0, 1.0}
    if case.kind == "pinf-ninf":  # (not empty: see the table's docstring)
        assert (ok == 1.0).sum() > 0 and (ok == 0.0).sum() > 0
    if case.kind in qc.EXACT_KINDS:
        assert qc.is_exact(v, q), "the table calls this kind exact"
    if case.kind in qc.OVERFLOW_KINDS:
        assert np.isfinite(q).all() and not np.isfinite(q.astype(np.float16)).all()
    elif case.kind not in qc.NONFINITE_KINDS:
        with np.errstate(over="ignore"):
            assert np.isfinite(q.astype(np.float16)).all()
    assert not _rejected(v, q, s, case), "the checker rejects the oracle's own answer"
    if case.kind == "zero":
        n = qc.answer(s, case.k, case.thr)[0].size
        assert n == (0 if case.thr == qc.HALF_UP else (min(case.k, qc.ROWS) if case.k else qc.ROWS))


def test_overflow_teeth_the_split_model_is_rejected():
    """edge-65520, over-opposed, over-all: the split planes' answer must not pass (k = 10; over-opposed also item for item at k = 300)"""
    seen = set()
    for c in CASES:
        if c.kind in ("edge-65520", "over-one", "over-opposed", "over-all") and c.k in (10, 300) and c.thr is None:
            v, q = _inputs(c)
            assert _rejected(v, q, qc.split_model_scores(v, q), c), c.name
            seen.add(c.kind)
    assert seen == {"edge-65520", "over-one", "over-opposed", "over-all"}


def test_split_model_is_accepted_where_it_is_exact():
    """edge-65504, edge-65519, every scale, the zero and subnormal queries, and the truly non-finite ones (whose fp32 answer the split
    computes: inf and NaN highs get a zero low part)"""
    kinds = ("edge-65504", "edge-65519", "zero", "f32-subnormal", "row-times-3", "neg-row") + tuple(qc.SCALES) + qc.NONFINITE_KINDS
    seen = set()
    for c in CASES:
        if c.kind in kinds:
            v, q = _inputs(c)
            assert not _rejected(v, q, qc.split_model_scores(v, q), c), c.name
            seen.add(c.kind)
    assert seen == set(kinds)


def test_a_filter_score_leaking_into_an_answer_is_seen():
    """float16(q) alone: rejected for at least one scale at k = 10 on every (width, dtype)"""
    for dtype, dims in qc.DIMS.items():
        for dim in dims:
            hit = [c.name for c in CASES if c.kind in qc.SCALES and c.k == 10 and c.thr is None and (c.dim, c.dtype) == (dim, dtype)
                   and _rejected(*_inputs(c), qc.q16_model_scores(*_inputs(c)), c)]
            assert hit, (dim, dtype)


def test_batches_place_the_edge_queries():
    qs, thrs, slots = qc.batch("gauss", 64, "fp16", 70, qc.kinds_for("gauss"), 10)
    assert qs.shape == (70, 64) and thrs.shape == (70,)
    for s in (0, 31, 32, 63, 64, 69):
        assert slots[s].kind != "unit", s
    assert any(s.kind == "unit" for s in slots)
    assert {float(t) for t in thrs} >= {0.0, 0.5, 1.0}
    _, _, slots = qc.batch("gauss-z", 64, "fp16", 40, qc.kinds_for("gauss-z"), 10, all_edge=True)
    assert all(s.kind != "unit" for s in slots)
    assert {s.kind for s in slots} >= set(qc.NONFINITE_KINDS) | set(qc.OVERFLOW_KINDS)
