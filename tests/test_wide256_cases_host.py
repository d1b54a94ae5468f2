"""CPU suite: the inputs of tests/test_gpu_wide256_shapes.py prove what they are there to prove, and the kernel its table expects is the
kernel the library picks.

Coverage is a condition on the inputs, computed from the float64 oracle alone: the top 256 of 256 queries over a few hundred rows must put at
least one returned (row, query) pair into every class of a 320-row x 256-query tile -- every tile row against every 16-query fragment, every
16-row fragment against every query lane.  Then a wrong accumulator-to-row or lane-to-query mapping in ANY block class of the filter tile drops
a row some query must return, and the GPU suite sees it.  (With k = 32 about a fifth of the classes hold no returned pair.)  A case whose inputs
do not meet the condition gets other inputs, not another condition."""

import numpy as np
import pytest

from tests import wide256_cases as wc
from typeagent_py_amd import _native

DENSE = [c for c in wc.CASES if c.dense]


@pytest.mark.parametrize("case", DENSE, ids=[c.name for c in DENSE])
def test_returned_pairs_cover_every_block_class(case):
    assert case.nq == 256 and case.k == 256 and case.thr == "zero"
    v, _, qs = wc.case_inputs(case)
    top = wc.oracle_topk_rows(v, qs, case.k)
    assert top.shape == (case.nq, min(case.k, case.rows))
    holes1, holes2 = wc.coverage_holes(case.rows, top)
    assert not holes1, f"{case.name}: no returned pair in (row mod 320, query // 16 mod 16) classes {holes1[:8]} ({len(holes1)} in all)"
    assert not holes2, f"{case.name}: no returned pair in (row mod 320 // 16, query mod 256) classes {holes2[:8]} ({len(holes2)} in all)"


def test_coverage_condition_notices_a_sparse_answer():
    """k = 32 over 643 rows leaves classes empty: the condition above is not vacuous."""
    case = next(c for c in wc.CASES if c.name == "width-f16-d64")
    v, _, qs = wc.case_inputs(case)
    holes1, holes2 = wc.coverage_holes(case.rows, wc.oracle_topk_rows(v, qs, 32))
    assert holes1 and holes2


def test_planted_rows_lead_their_queries():
    """a planted row is its query's best hit by the float64 oracle (group 2: the last row and the last row of every complete 80-row half)"""
    for case in wc.CASES:
        where = wc.planted(case)
        if not where:
            continue
        v, _, qs = wc.case_inputs(case)
        assert len(set(where.values())) == len(where) and max(where.values()) < case.rows
        if case.plant == "halves":
            assert where[0] == case.rows - 1
            assert sorted(set(where.values()) - {case.rows - 1}) == [r for r in range(79, case.rows - 1, 80)]
        top1 = wc.oracle_topk_rows(v, qs[sorted(where)], 1)[:, 0]
        assert top1.tolist() == [where[q] for q in sorted(where)], case.name


def test_table_holds_what_the_suite_is_for():
    by = {}
    for c in wc.CASES:
        by.setdefault(c.group, []).append(c)
    assert sorted(c.dim for c in by["width"] if c.dtype == "fp16" and not c.padded) == [64, 128, 192, 320, 960, 1536, 3072, 4096]
    assert sorted(c.dim for c in by["width"] if c.dtype == "fp16" and c.padded) == [33, 100, 130, 1000]
    assert sorted(c.dim for c in by["width"] if c.dtype == "fp32") == [64, 80, 192, 1536]
    assert all(c.rows == 643 and c.nq == 256 and c.k == 256 for c in by["width"])
    for d in (64, 192):
        assert sorted(c.rows for c in by["tail"] if c.dim == d) == sorted(320 * t + r for t in (0, 2) for r in wc.ROW_TAILS)
    assert all(c.splits == ((0, 1, 3) if c.rows > 320 else (0,)) for c in by["tail"])
    # one workgroup over the whole corpus appends more keys per query than a buffer holds between compactions
    assert all(c.rows > wc.CAPW - wc.TILE_ROWS and 1 in c.splits and 0 in c.splits for c in by["compact"])
    assert sorted({c.nq for c in by["qtail"]}) == [65, 129, 143, 255, 256, 257, 513] and {c.k for c in by["qtail"]} == {32, 256}
    assert sorted(c.k for c in by["kthr"] if c.thr == "zero") == [1, 64, 65, 256] and {c.thr for c in by["kthr"]} == {"zero", "fifth", "mixed"}
    for c in by["ladder"]:
        b = wc.case_ladder_bounds(c)
        assert len(b) - 1 >= 3 and 12_000 <= c.rows <= 20_000, (c.name, b)
    assert by["base"][0].base + by["base"][0].rows == 2**32 - 2


def test_planner_expectations():
    """which kernel the table expects: the 256-query tile follows mfma_shape, the 128-query tile stays on 32x32x16"""
    assert _native.plan_filter_shape(16, 256) == 16
    assert _native.plan_filter_shape(32, 256) == 32
    assert _native.plan_filter_shape(16, 128) == 32
