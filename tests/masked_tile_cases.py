"""The case table of tests/test_gpu_masked_tile.py and of its CPU twin tests/test_masked_tile_host.py: the MASKED instantiations of the 32/64-query
tile (`skinny_scan_kernel<..., MASKED = true>`, csrc/tavb_mfma_skinny.hip) behind tavb_search_masked_device, in the style of tests/skinny_cases.py,
whose input builders, route options and Python mirrors of the library's rules it reuses.

What the masked form adds to the tile is one scalar load per 32-row block of the epilogue (the block's word of the mask), a skip of blocks whose
word is zero, and one bit test per admitted row; the route adds the row span (the phases run over [first allowed row rounded down to 256,
last allowed row]) and the per-phase word offset.  So the table varies the mask against the geometry of a tile -- single rows at both ends of a
tile and of the corpus, alternating bits, whole words cleared in every wave's part of a tile, a contiguous range with unaligned ends, a last
word with garbage behind the corpus -- at every row tail around a word and a tile, both K steps, both dtypes, both query tiles, every staging
variant, forced row ranges (compaction between tiles at threshold 0, empty ranges, a range count that is no multiple of 8) and a ladder of
several phases.  Small corpora and k = 64 for the reason skinny_cases gives: every query returns a large share of the allowed rows, so an
ignored or shifted mask bit is a wrong answer in nearly every query.

The table's own claims (tests/test_masked_tile_host.py asserts them on the CPU, from the float64 oracle alone): with a partial mask at
threshold 0 every query's UNMASKED top k holds a disallowed row -- a kernel that ignores the mask fails every query -- and every one of the 8
word positions of a 256-row tile holds, somewhere in the table, both a returned allowed row and a disallowed row of an unmasked top k.

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import skinny_cases as sc

ROUTE_OPTS = (*sc.ROUTE_OPTS, ("mask_tile", 2))
WORD = 32  # rows per word of a mask


@dataclass(frozen=True)
class Case:
    name: str
    group: str  # "width", "rows", "mask", "batch", "splits", "ladder"
    dtype: str
    rows: int
    dim: int
    mask: str  # see case_mask
    nq: int = 64
    k: int = 64
    thr: str = "zero"  # "zero", "half" (0.5 for every query), "mixed" (one threshold per query)
    splits: tuple = (0,)
    opts: tuple = ()
    span: str = "tight"  # "tight": (first, last) allowed row, as RowMask gives it; "whole": (0, rows - 1)
    seed: int = 0

    @property
    def f32(self) -> bool:
        return self.dtype == "fp32"

    @property
    def inputs_case(self) -> sc.Case:
        """the skinny_cases case whose input builder makes this case's rows and queries"""
        return sc.Case(self.name, "masked", self.dtype, self.rows, self.dim, nq=self.nq, k=self.k, seed=self.seed)


def case_inputs(case: Case):
    """-> (the values the kernel multiplies, float32 [rows, dim]; the rows as stored; the queries float32 [nq, dim]) -- skinny_cases.case_inputs"""
    return sc.case_inputs(case.inputs_case)


@functools.lru_cache(maxsize=8)
def case_mask(case: Case) -> np.ndarray:
    """the allow-mask of a case, bool [rows]"""
    n, kind = case.rows, case.mask
    r = np.arange(n)
    rng = np.random.default_rng(case.seed + 77)
    if kind == "all":
        m = np.ones(n, dtype=bool)
    elif kind == "none":
        m = np.zeros(n, dtype=bool)
    elif kind.startswith("one@"):  # a single row: "one@last" or "one@<row>"
        m = np.zeros(n, dtype=bool)
        m[n - 1 if kind == "one@last" else int(kind[4:])] = True
    elif kind == "alt":
        m = r % 2 == 0
    elif kind in ("wordclear", "wordkeep"):
        # one whole 32-row word cleared in every wave's part of a 256-row tile (a wave owns 64 rows = two words; of a half tile, one word): words
        # 0, 3, 4, 7 of the tile -- and the complement, in which only those words are allowed
        cleared = np.isin((r % sc.TILE_ROWS) // WORD, (0, 3, 4, 7))
        m = ~cleared if kind == "wordclear" else cleared
    elif kind == "rand50":
        m = rng.random(n) < 0.5
    elif kind == "rand2":
        m = rng.random(n) < 0.02
        m[rng.integers(n)] = True  # (never empty)
    elif kind == "nobest":  # random 50 % less every query's float64-best row: the unmasked top k of every query holds a disallowed row whatever k
        m = rng.random(n) < 0.5
        v, _, qs = case_inputs(case)
        m[np.argmax(np.asarray(v, dtype=np.float64) @ np.asarray(qs, dtype=np.float64).T, axis=0)] = False
    elif kind.startswith("range"):  # "range300-700": rows [300, 700), unaligned ends
        lo, hi = (int(x) for x in kind[5:].split("-"))
        m = (r >= lo) & (r < hi)
    else:
        raise ValueError(kind)
    return m


def case_words(case: Case, garbage: bool = False) -> np.ndarray:
    """the mask in the library's bit form, uint32 [(rows + 31) // 32]: row r = bit r & 31 of word r >> 5.  garbage: the bits at or beyond `rows`
    in the last word set to 1 (they "may hold anything")"""
    m = case_mask(case)
    n_words = (case.rows + WORD - 1) // WORD
    padded = np.zeros(n_words * WORD, dtype=bool)
    padded[: case.rows] = m
    if garbage:
        padded[case.rows:] = True
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def case_garbage(case: Case) -> bool:
    """cases that hand the library a last word with ones behind the corpus: every case whose mask says "tailones" by name, and all others with an odd
    seed -- the answer may not depend on those bits anywhere"""
    return case.name.endswith("tailones") or case.seed % 2 == 1


def case_span(case: Case) -> tuple[int, int] | None:
    """(first, last) row handed to the library; None: the mask is empty (first > last)"""
    flat = np.flatnonzero(case_mask(case))
    if len(flat) == 0:
        return None
    return (0, case.rows - 1) if case.span == "whole" else (int(flat[0]), int(flat[-1]))


def span_rows(case: Case) -> tuple[int, int]:
    """[begin, end) of the rows the tile scans: the span with its begin rounded down to a multiple of 256"""
    first, last = case_span(case)
    return first // sc.TILE_ROWS * sc.TILE_ROWS, last + 1


def case_phase_starts(case: Case, splits: int = 1) -> list[int]:
    """the corpus row every phase of the ladder starts at (tavb_route.hip::run_tile_ladder over the span)"""
    begin, end = span_rows(case)
    o = dict(case.opts)
    return [begin + b for b in sc.phase_bounds(end - begin, splits, o.get("mfma_sample_rows", 0), o.get("mfma_ladder", 4))[:-1]]


def case_thresholds(case: Case) -> np.ndarray:
    from typeagent_py_amd import _native

    pattern = {"zero": [0.0], "half": [0.5], "mixed": [0.0, 0.5, float("nan"), 1.5, 0.52]}[case.thr]
    return np.array([_native.f32_threshold(pattern[i % len(pattern)]) for i in range(case.nq)], dtype=np.float32)


def runs(case: Case) -> list[sc.Run]:
    """every way a case is run (skinny_cases.runs): the first 32 queries and the whole batch, on whole-line widths the 32 again under mfma_sched 8,
    6, 5 and 9, all under every mfma_splits of the case"""
    return sc.runs(case.inputs_case if case.splits == (0,) else sc.Case(case.name, "masked", case.dtype, case.rows, case.dim, nq=case.nq, k=case.k,
                                                                        splits=case.splits, seed=case.seed))


ONE_PHASE = sc.ONE_PHASE
LADDER_OPTS = sc.LADDER_OPTS  # mfma_sample_rows = 256, mfma_ladder = 4: phases of 256, 1024 and the rest of a span of 2048+ rows
WIDTHS = (("fp16", 64), ("fp16", 96), ("fp16", 1536), ("fp32", 64), ("fp32", 48), ("fp32", 1536))  # fp16 64: ONE 128-byte step; 96 / 48: 64-byte steps
PAIR = (("fp16", 96), ("fp32", 64))  # one half-line and one whole-line width, one per dtype
ROWS = (1, 31, 32, 33, 255, 256, 257, 600, 1300)
MASKS = ("all", "none", "one@0", "one@255", "one@256", "one@last", "alt", "wordclear", "wordkeep", "rand50", "rand2")


def _seed(i: int) -> int:
    return 900_000 + 16 * i


def _table() -> list[Case]:
    out: list[Case] = []

    def add(name, group, dt, rows, dim, mask, **kw):
        out.append(Case(f"{group}-{dt}-d{dim}-{name}", group, dt, rows, dim, mask, seed=_seed(len(out)) + kw.pop("odd", 0), **kw))

    for dt, d in WIDTHS:
        add("rand50", "width", dt, 600, d, "rand50")
    for dt, d in PAIR:
        for n in ROWS:
            add(f"rows{n}", "rows", dt, n, d, "alt", odd=1)  # (odd seed: garbage behind the corpus in the last word)
    for dt, d in (("fp16", 64), ("fp32", 64)):
        for mk in MASKS:
            add(mk, "mask", dt, 600, d, mk)
        add("range300-700", "mask", dt, 1300, d, "range300-700")
        add("tailones", "mask", dt, 600, d, "rand50")  # 600 = 18 words + 24 rows: 8 bits of garbage
    for dt, d in PAIR:
        add("nq65", "batch", dt, 600, d, "rand50", nq=65)
        add("k10", "batch", dt, 600, d, "nobest", k=10)
        add("thr-half", "batch", dt, 600, d, "rand50", thr="half")
        add("thr-mixed", "batch", dt, 600, d, "rand50", thr="mixed")
    # forced row ranges over 1300 rows = six tiles, ONE phase: 1 = one workgroup walks all six and compacts at threshold 0 (650 allowed rows per
    # query against buffers of 512); 8 = ranges of one tile, the last two empty; 5 = no multiple of 8
    for dt, d in (*PAIR, ("fp16", 64)):
        add("rand50", "splits", dt, 1300, d, "rand50", splits=(1, 8, 5, 0), opts=ONE_PHASE)
    add("alt", "splits", "fp32", 1300, 64, "alt", splits=(1, 5), opts=ONE_PHASE, odd=1)
    # several phases over 2600 rows: the word offset of every phase.  rand50: phases start at rows 0, 256, 1280; range300-2500: the span starts at
    # 256 and is 2244 rows, two phases, at rows 256 and 512; late ("whole" span, rows from 1400 on): the first two phases hold no allowed row and seed nothing
    for dt, d in PAIR:
        add("rand50", "ladder", dt, 2600, d, "rand50", opts=LADDER_OPTS)
        add("range300-2500", "ladder", dt, 2600, d, "range300-2500", opts=LADDER_OPTS, odd=1)
        add("late", "ladder", dt, 2600, d, "range1400-2600", opts=LADDER_OPTS, span="whole")
    return out


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)


def partial(case: Case) -> bool:
    m = case_mask(case)
    return bool(m.any() and not m.all())


def oracle_tops(case: Case) -> tuple[np.ndarray, np.ndarray]:
    """by the float64 oracle: (every query's unmasked top k rows [nq, min(k, rows)]; every query's top k among the allowed rows, as corpus rows
    [nq, min(k, allowed)])"""
    v, _, qs = case_inputs(case)
    m = case_mask(case)
    flat = np.flatnonzero(m)
    unmasked = sc.oracle_topk_rows(v, qs, case.k)
    masked = flat[sc.oracle_topk_rows(v[flat], qs, case.k)] if len(flat) else np.zeros((case.nq, 0), dtype=np.int64)
    return unmasked, masked
