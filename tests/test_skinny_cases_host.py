"""CPU suite: the table of tests/test_gpu_skinny_shapes.py (tests/skinny_cases.py) holds what it claims, with no engine.

The kernel a run expects is computed by Python mirrors of `skinny_supported`, `skinny_line_steps`, `skinny_variant` and `skinny_kernel_id`
(csrc/tavb_mfma_skinny.hip); the GPU suite then compares the library's own `last_skinny_kernel` with it after every call, so a mirror that
drifts from the library fails there.  Coverage is a condition on the inputs, computed from the float64 oracle alone: the top 64 of 64 (and of
the first 32) queries over a few hundred rows must put a returned (row, query) pair into every class of a 256-row (and 128-row) tile -- every
tile row against every 32-query block, every 32-row block against every query lane.  A case whose inputs do not meet the condition gets
another seed, not another condition."""

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import skinny_cases as sc

DENSE = [c for c in sc.CASES if c.dense]
BY_GROUP: dict = {}
for _c in sc.CASES:
    BY_GROUP.setdefault(_c.group, []).append(_c)


def test_names_are_unique_and_every_case_is_the_tiles():
    assert len({c.name for c in sc.CASES}) == len(sc.CASES)
    for c in sc.CASES:
        assert sc.skinny_supported(c.dim, c.k, c.f32), c.name
        assert c.rows <= 2563 and c.nq <= 200


def test_mirrors_of_the_dispatch():
    """the values of `last_skinny_kernel` by the rule of csrc/tavb_mfma_skinny.hip"""
    assert sc.kernel_id(1536, False, 32) == 12832 and sc.kernel_id(1536, True, 64) == 12864
    assert sc.kernel_id(96, False, 32) == 6432 and sc.kernel_id(16, True, 64) == 6464
    assert sc.kernel_id(1536, False, 32, 8) == 22832 and sc.kernel_id(1536, True, 32, 6) == 32832 and sc.kernel_id(1536, False, 32, 5) == 52832
    assert sc.kernel_id(1536, False, 32, 9) == 6432 and sc.kernel_id(1536, False, 32, 7) == 12832
    assert sc.kernel_id(1536, False, 64, 8) == 12864 and sc.kernel_id(1536, False, 64, 5) == 12864  # the 64-query tile keeps the ring
    assert sc.kernel_id(192, False, 32, 5) == 12832  # three K steps: no multiple of the register ring
    assert sc.kernel_id(96, False, 32, 8) == 6432 and sc.kernel_id(96, False, 32, 6) == 6432  # half-line widths have the ring only


@pytest.mark.parametrize("case", sc.CASES, ids=[c.name for c in sc.CASES])
def test_runs_of_a_case(case):
    """both query tiles, every mfma_splits, and on whole-line widths the four measurement schedules with the kernel each must report"""
    runs = sc.runs(case)
    line = sc.line_steps(case.dim, case.f32)
    step = 128 if line else 64
    assert case.row_bytes % step == 0 and sc.k_steps(case) == case.row_bytes // step
    for splits in case.splits:
        mine = [r for r in runs if r.splits == splits]
        plain = [r for r in mine if r.sched == 0]
        assert [r.nq for r in plain] == ([case.nq] if case.nq <= 32 else [32, case.nq])
        for r in plain:
            assert r.kernel == step * 100 + (32 if r.nq <= 32 else 64), (case.name, r)
        sched = {r.sched: r for r in mine if r.sched}
        if not line:
            assert not sched
            continue
        assert sorted(sched) == [5, 6, 8, 9] and all(r.nq == min(case.nq, 32) for r in sched.values())
        assert sched[8].kernel == 22832 and sched[6].kernel == 32832 and sched[9].kernel == 6432
        assert sched[5].kernel == (52832 if sc.k_steps(case) % 4 == 0 else 12832), case.name  # (fewer or odd steps: the ring, asserted as such)


def test_table_runs_every_instantiation():
    seen = {(c.dtype, r.kernel) for c in sc.CASES for r in sc.runs(c)}
    assert seen == sc.ALL_KERNELS
    forced = {c.dtype for c in sc.CASES for r in sc.runs(c) if r.sched == 9}
    assert forced == {"fp16", "fp32"}  # the forced 64-byte step on a whole-line width
    for c in BY_GROUP["tail"] + BY_GROUP["empty"] + BY_GROUP["compact"] + BY_GROUP["ladder"]:
        assert {r.kernel for r in sc.runs(c)} >= ({12832, 12864, 22832, 32832, 6432} if sc.line_steps(c.dim, c.f32) else {6432, 6464}), c.name


def test_table_holds_what_the_suite_is_for():
    width = BY_GROUP["width"]
    assert all(c.rows == 643 and c.nq == 64 and c.k == 64 for c in width)

    def steps(dtype, line):
        return sorted(sc.k_steps(c) for c in width if c.dtype == dtype and sc.line_steps(c.dim, c.f32) == line)

    assert sorted(c.dim for c in width if c.dtype == "fp16") == [32, 64, 96, 128, 160, 192, 256, 320, 1536, 1568, 3072]
    assert sorted(c.dim for c in width if c.dtype == "fp32") == [16, 32, 48, 64, 80, 96, 128, 160, 784, 1536]
    assert steps("fp16", True) == [1, 2, 3, 4, 5, 24, 48] and steps("fp16", False) == [1, 3, 5, 49]
    assert steps("fp32", True) == [1, 2, 3, 4, 5, 48] and steps("fp32", False) == [1, 3, 5, 49]
    # below, on and above every ring depth (2, 3, 4 slots) and the register ring (4 steps, which runs on multiples of 4 only)
    for dtype in ("fp16", "fp32"):
        assert {1, 2, 3, 4, 5} <= set(steps(dtype, True)) and {1, 3, 5} <= set(steps(dtype, False))
        assert [s for s in steps(dtype, True) if s % 4 == 0][0] == 4
    for dt, d in sc.TAIL_WIDTHS:
        assert sorted(c.rows for c in BY_GROUP["tail"] if (c.dtype, c.dim) == (dt, d)) == sorted(256 * t + r for t in (0, 2) for r in sc.ROW_TAILS)
    assert {sc.line_steps(d, dt == "fp32") for dt, d in sc.TAIL_WIDTHS if dt == "fp32"} == {True, False}
    assert {sc.line_steps(d, dt == "fp32") for dt, d in sc.TAIL_WIDTHS if dt == "fp16"} == {True, False}
    assert all(c.splits == ((0, 1, 3) if c.rows > 256 else (0,)) and c.plant == "blocks" for c in BY_GROUP["tail"])
    for g in (4, 8, 32, 64, 128, 256):  # one below, on and one above every granularity of the epilogue
        assert {g - 1, g, g + 1 if g < 256 else 1} <= set(sc.ROW_TAILS)
    assert {c.nq for c in BY_GROUP["qtail"] if c.f32} == {3, 31, 32, 33, 63, 64, 65, 96, 129, 200}
    assert {c.nq for c in BY_GROUP["qtail"] if not c.f32} == {3, 31, 33, 63, 64}
    for dt in ("fp16", "fp32"):
        kthr = [c for c in BY_GROUP["kthr"] if c.dtype == dt]
        assert sorted(c.k for c in kthr if c.thr == "zero") == [1, 2, 32, 63, 64] and {c.thr for c in kthr} == {"zero", "fifth", "mixed"}
        assert all(c.rows == 2563 for c in kthr)
    base = BY_GROUP["base"][0]
    assert base.base + base.rows == 2**32 - 2


def test_mirror_of_the_phase_bounds():
    """tavb_route.hip::ladder_bounds for this tile: a forced single range of 1024 rows and more is a seeding tile + the rest by default"""
    assert sc.phase_bounds(1283, 1) == [0, 256, 1283] and sc.phase_bounds(1283, 1, -1) == [0, 1283]
    assert sc.phase_bounds(1023, 1) == [0, 1023] and sc.phase_bounds(1024, 1) == [0, 256, 1024]
    assert sc.phase_bounds(768, 3) == [0, 768] and sc.phase_bounds(3072, 3) == [0, 768, 3072]
    assert sc.phase_bounds(2563, 8, 256, 4) == [0, 256, 1280, 2563] and sc.phase_bounds(2563, 8, 256, 0) == [0, 256, 2563]
    assert sc.phase_bounds(2_048_000, 8) == [0, 2048, 26624, 2_048_000]


def test_ladder_cases_have_three_phases_and_planted_bounds():
    for c in BY_GROUP["ladder"]:
        b = sc.case_ladder_bounds(c)
        assert b == [0, 256, 1280, 2563], (c.name, b)
        where = sc.planted(c)
        assert where[0] == 5 and where[1] == c.rows - 3 and [where[2], where[3]] == b[1:-1]


def test_forced_row_ranges_run_in_one_phase():
    """a run under a forced mfma_splits is ONE launch over the ranges `row_ranges` gives -- no seeding phase in front of it (the ladder group
    aside, which asks for its phases); the GPU suite asserts the launch counts"""
    n = 0
    for c in sc.CASES:
        for splits in c.splits:
            if splits > 0 and c.group != "ladder":
                assert sc.case_phase_bounds(c, splits) == [0, c.rows], (c.name, splits)
                n += 1
    assert n == 2 * 4 * len(sc.ROW_TAILS) + 3 * 4 + 12


def test_empty_range_cases_leave_ranges_empty():
    for c in BY_GROUP["empty"]:
        for s in c.splits:
            assert s == 0 or sc.case_phase_bounds(c, s) == [0, c.rows]  # the ranges below are those of the one launch
        if c.rows == 300:
            assert c.splits[:2] == (8, 5)
            for s in (8, 5):
                rr = sc.row_ranges(c.rows, s)
                assert rr[0] == (0, 256) and rr[1] == (256, 300) and all(b >= e for b, e in rr[2:]) and len(rr) == s
        else:
            assert c.rows == 257 and c.splits[0] == 2 and sc.row_ranges(257, 2) == [(0, 256), (256, 257)]
    assert {c.rows for c in BY_GROUP["empty"]} == {300, 257}


@pytest.mark.parametrize("case", BY_GROUP["compact"], ids=[c.name for c in BY_GROUP["compact"]])
def test_compact_cases_compact_between_tiles(case):
    """One workgroup, one phase, threshold 0, by the float64 oracle: EVERY query's buffer passes the limit before the last tile and is cut to
    its best k -- with 256-row tiles after the second tile, exactly full (CAP); with 128-row tiles after the fourth, at CAP keys against the
    limit of CAP - 128 -- and no buffer ever holds more than CAP keys."""
    assert case.splits == (1, 0) and case.thr == "zero" and case.rows == 1283 and case.nq == 64
    assert sc.case_phase_bounds(case, 1) == [0, case.rows] and sc.row_ranges(case.rows, 1) == [(0, case.rows)]
    for tile_rows, first in ((sc.TILE_ROWS, 1), (sc.HALF_ROWS, 3)):
        last_tile = (case.rows + tile_rows - 1) // tile_rows - 1
        for q, trace in enumerate(sc.compaction_trace(case, tile_rows)):
            assert trace and trace[0] == (first, sc.CAP), (case.name, tile_rows, q, trace)
            assert trace[0][1] > sc.CAP - tile_rows and all(t < last_tile for t, _ in trace)


def test_compact_group_holds_every_k():
    for dt, d in sc.TAIL_WIDTHS:
        assert sorted(c.k for c in BY_GROUP["compact"] if (c.dtype, c.dim) == (dt, d)) == [1, 33, 64]


def test_planted_rows_lead_their_queries():
    """a planted row is its query's first hit by the float64 oracle"""
    n = 0
    for case in sc.CASES:
        where = sc.planted(case)
        if not where:
            continue
        v, _, qs = sc.case_inputs(case)
        assert len(set(where.values())) == len(where) and max(where.values()) < case.rows and max(where) < min(case.nq, 32)
        if case.plant == "blocks":
            tile0 = (case.rows - 1) // 256 * 256
            assert where[0] == case.rows - 1
            assert sorted(set(where.values()) - {case.rows - 1}) == [r for r in range(tile0 + 31, case.rows - 1, 32)]
        top1 = sc.oracle_topk_rows(v, qs[sorted(where)], 1)[:, 0]
        assert top1.tolist() == [where[q] for q in sorted(where)], case.name
        n += 1
    assert n == len(BY_GROUP["tail"]) + len(BY_GROUP["ladder"])


@pytest.mark.parametrize("case", DENSE, ids=[c.name for c in DENSE])
def test_returned_pairs_cover_every_block_class(case):
    assert case.nq == 64 and case.k == 64 and case.thr == "zero" and case.rows > 256
    for what, (holes1, holes2) in sc.case_holes(case).items():
        assert not holes1, f"{case.name}, {what}: no returned pair in (row mod tile, query // 32) classes {holes1[:8]} ({len(holes1)} in all)"
        assert not holes2, f"{case.name}, {what}: no returned pair in (row mod tile // 32, query mod 64) classes {holes2[:8]} ({len(holes2)} in all)"


def test_dense_cases_are_the_ones_the_condition_is_for():
    assert {c.name for c in DENSE} == {c.name for c in sc.CASES if (c.group == "width" or (c.group == "compact" and c.k == 64) or
                                                                   (c.group == "tail" and c.rows > 512))}


def test_coverage_condition_notices_a_sparse_answer():
    """k = 8 over 643 rows leaves classes empty: the condition above is not vacuous."""
    case = next(c for c in sc.CASES if c.name == "width-fp32-d64")
    v, _, qs = sc.case_inputs(case)
    holes1, holes2 = sc.coverage_holes(case.rows, sc.oracle_topk_rows(v, qs, 8))
    assert holes1 and holes2


def test_qtail_single_lookups_are_determinate():
    """the queries whose batch entry must equal the single lookup's ordinals (another kernel, another summation order) have no float64 near tie
    among their best k + 1 rows: eight times the tie width of the oracle, 2e-6, where float32 arithmetic over 64 or 96 terms is good to 1e-7"""
    for case in BY_GROUP["qtail"]:
        v, _, qs = sc.case_inputs(case)
        singles = sc.single_queries(case)
        assert case.nq - 1 in singles and (case.nq - 1) // sc.query_tile(case.nq) * sc.query_tile(case.nq) in singles
        for qi in singles:
            s = np.sort(vo.scores_f64(v, qs[qi]))[::-1][: case.k + 1]
            assert float(np.min(-np.diff(s))) >= 8 * vo.TIE_EPS, (case.name, qi)
