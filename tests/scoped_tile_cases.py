"""TEST INFRASTRUCTURE -- the case table of the scoped batches on the 32/64-query tile (one scope per query in the tile's admission path:
the SCOPED instantiations of `skinny_scan_kernel`, csrc/tavb_mfma_skinny.hip, behind tavb_search_scoped_tile), shared by
tests/test_gpu_scoped_tile.py (the device) and tests/test_scoped_tile_host.py (its CPU twin).

A case = a corpus (width, dtype), a row count, a batch size, a max_hits, a family of scopes (tests/scoped_batch_cases.py: `case_scopes`) and
a kind of thresholds, plus the engine options and the forced row ranges it runs under.  Corpora, row counts, max_hits and thresholds rotate
through the table so that every family meets every batch size and every corpus meets every row count; the inputs are those of
tests/skinny_cases.py (Gaussian unit rows and queries).

What the per-query form adds to the tile: per (32-row block, 32-query block) 32 plane words through the scalar data path, a skip of blocks
whose words are all zero, and one 64-bit AND per row pair -- lanes 0-31 take the word of row r, lanes 32-63 the word of row r + 4.  What the
route adds: the planes (a 32 x 32 bit transpose per 32-row block, `planes_numpy` restates it), their offset per ladder phase and per query
block, and the waves.  So the batches stand around the 32- and 64-query tile (1, 31, 32, 33, 64, 65, 97: one block, two, a second query tile, an
odd block in the last tile), the rows around a mask word and a 256-row tile, and the scopes differ BETWEEN queries of one block (disjoint,
nested, random) -- a plane of the wrong block, the wrong half of a row pair or a stale phase offset is a wrong answer.

A plain module (no test, no fixture)."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import scoped_batch_cases as sb
from tests import skinny_cases as sc

ROUTE_OPTS = (*sc.ROUTE_OPTS, ("scope_tile", 2))
ROWS = (1, 31, 32, 33, 255, 256, 257, 1300, 4099)
BATCHES = (1, 31, 32, 33, 64, 65, 97)
MAX_HITS = (1, 10, 64)
FAMILIES = sb.FAMILIES
THR_CYCLE = sb.THR_CYCLE
# 64-byte rows (64-byte K steps); whole-line rows, on which the 32-query runs repeat under mfma_sched 8 / 6 / 5 / 9; one real width
SMALL = (("fp32", 16), ("fp16", 32), ("fp32", 32), ("fp16", 64))
WIDE = ("fp16", 1536)


@dataclass(frozen=True)
class Case:
    name: str
    group: str  # "family", "rows", "wide", "ladder", "splits"
    dtype: str  # "fp32" / "fp16"
    dim: int
    rows: int
    nq: int
    k: int
    family: str
    thresholds: str  # "uniform" (0 for every query) / "per_query" (THR_CYCLE)
    splits: tuple = (0,)
    opts: tuple = ()
    seed: int = 0

    @property
    def f32(self) -> bool:
        return self.dtype == "fp32"

    @property
    def inputs_case(self) -> sc.Case:
        return sc.Case(self.name, "scoped", self.dtype, self.rows, self.dim, nq=self.nq, k=self.k, splits=self.splits, seed=self.seed)


def _table() -> list[Case]:
    out: list[Case] = []

    def add(group, dt, dim, rows, nq, k, family, thr, **kw):
        i = len(out)
        out.append(Case(f"{group}-{dt}-d{dim}-r{rows}-q{nq}-k{k}-{family}-{thr}", group, dt, dim, rows, nq, k, family, thr, seed=940_000 + 16 * i + (i // 3) % 2, **kw))

    i = 0
    for nq in BATCHES:  # every family at every batch size: 70 cases
        for family in FAMILIES:
            dt, dim = SMALL[(i + i // 7) % len(SMALL)]
            add("family", dt, dim, ROWS[(i + i // 10) % len(ROWS)], nq, MAX_HITS[(i + i // 7) % len(MAX_HITS)], family, "per_query" if (i + i // 10) % 3 == 0 else "uniform")
            i += 1
    j = 0
    for dt, dim in SMALL:  # every corpus at every row count: 36 cases, scopes that differ between the queries of a block
        for rows in ROWS:
            add("rows", dt, dim, rows, BATCHES[2 + j % 5], MAX_HITS[1 + j % 2], ("random50%", "nested", "disjoint", "first_row", "last_row")[j % 5],
                "per_query" if j % 4 == 0 else "uniform")
            j += 1
    for nq, family in ((32, "random50%"), (33, "nested"), (65, "disjoint"), (97, "random50%")):  # 24 whole-line K steps: register staging runs
        add("wide", *WIDE, 1300, nq, 10, family, "uniform")
    add("wide", "fp32", 128, 1300, 32, 10, "random50%", "per_query")  # four whole-line K steps: register staging on fp32
    # several phases over 4099 rows (256, 1280, the rest): the plane offset of every phase; 97 queries: two query tiles, the second half empty
    for dt, dim in (("fp32", 32), ("fp16", 32)):
        add("ladder", dt, dim, 4099, 97, 64, "random50%", "uniform", opts=sc.LADDER_OPTS)
        add("ladder", dt, dim, 4099, 33, 10, "disjoint", "per_query", opts=sc.LADDER_OPTS)
    # forced row ranges over 1300 rows = six tiles, ONE phase: 1 = one workgroup walks all six and compacts at threshold 0; 8 = ranges of one
    # tile, the last two empty; 5 = no multiple of 8
    for dt, dim in (("fp32", 32), ("fp16", 32), ("fp16", 64)):
        add("splits", dt, dim, 1300, 65, 64, "random50%", "uniform", splits=(1, 8, 5, 0), opts=sc.ONE_PHASE)
    return out


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)


def case_inputs(case: Case):
    """-> (the values the kernel multiplies, float32 [rows, dim]; the rows as stored; the queries float32 [nq, dim]) -- skinny_cases.case_inputs"""
    return sc.case_inputs(case.inputs_case)


def case_scopes(case: Case) -> list[np.ndarray]:
    """one bool [rows] array per query (scoped_batch_cases.case_scopes: it reads rows, nq, family and seed)"""
    return sb.case_scopes(case)


def case_thresholds(case: Case) -> np.ndarray:
    """float32 [nq] as the engine takes them; THR_CYCLE's None (the class' default) is 0 here"""
    if case.thresholds == "uniform":
        return np.zeros(case.nq, dtype=np.float32)
    return np.array([THR_CYCLE[i % len(THR_CYCLE)] or 0.0 for i in range(case.nq)], dtype=np.float32)


def case_garbage(case: Case) -> bool:
    """cases that hand the library masks whose last word has ones behind the corpus: the bits "may hold anything" """
    return case.seed % 2 == 1


def scope_words(scope: np.ndarray, garbage: bool = False) -> np.ndarray:
    """a scope in the library's bit form, uint32 [(rows + 31) // 32]: row r = bit r & 31 of word r >> 5"""
    n = len(scope)
    padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
    padded[:n] = scope
    if garbage:
        padded[n:] = True
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def union_span(scopes) -> tuple[int, int] | None:
    """(first, last) row of the union of the scopes, as the class computes it from the handles' spans; None: every scope is empty"""
    rows = np.flatnonzero(np.logical_or.reduce(scopes))
    return (int(rows[0]), int(rows[-1])) if len(rows) else None


def plane_shape(n_masks: int, first: int, last: int) -> tuple[int, int, int]:
    """(blocks of 32 queries of the tile-padded batch, words per plane, first row of a plane): tavb_scope_planes' output layout"""
    begin = first // 256 * 256
    return (1 if n_masks <= 32 else 2 * ((n_masks + 63) // 64)), (last + 32) // 32 * 32 - begin, begin


def planes_numpy(scopes, first: int, last: int) -> np.ndarray:
    """`scope_planes_kernel` in numpy: uint32 [blocks, words], bit i of [b, r - begin] = scope 32 b + i holds row r, for begin <= r <= last"""
    blocks, words, begin = plane_shape(len(scopes), first, last)
    out = np.zeros((blocks, words), dtype=np.uint32)
    for q, s in enumerate(scopes):
        r = np.flatnonzero(s)
        r = r[(r >= begin) & (r <= last)]
        out[q // 32, r - begin] |= np.uint32(1 << (q % 32))
    return out


def runs(case: Case) -> list[sc.Run]:
    """every way a case is run (skinny_cases.runs): its first 32 queries and the whole batch, on whole-line widths the 32 again under
    mfma_sched 8, 6, 5 and 9, all under every mfma_splits of the case"""
    return sc.runs(case.inputs_case)
