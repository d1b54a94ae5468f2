"""The case table of tests/test_gpu_masked_wide.py and of its CPU twin tests/test_masked_wide_host.py: masked batches on the 128/256-query filter
tile (`mfma_scan_masked_kernel`, csrc/tavb_mfma_wide.hip) followed by exact rescoring -- `tavb_search_masked_wide`.

What the cases are for.  The route ends in the rescoring, so its answers must EQUAL the row-list route's (ordinals, float32 score bits, counts);
a wrong bit test in the filter shows as a missing row (a cleared bit read as set costs nothing: the rescoring never sees the mask, but the row
list's answer does not hold the row, so it shows too).  The corpora are 640 - 2600 rows, so the library's own choice at 256 queries is the
128-query tile (`mfma_query_tile_for`: a corpus this small gives a 256-query tile too few workgroups); the 256-query tile in its three forms is
therefore FORCED with `mfma_tile = 256` (VARIANTS), exactly as tests/test_gpu_wide256_shapes.py does, and `last_mfma_shape` says what ran.

`tile_reads_32` / `tile_reads_16` restate which mask word and bit every (wave, block or 80-row group, lane, register) of a tile tests, in both
MFMA shapes; the CPU twin checks them against the row each accumulator register holds and shows that the table admits and rejects a row at
every one of the 320 row positions of a tile (hence at every bit 0 .. 31 and both group offsets).

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests.synth import make_corpus, make_queries
from tests.wide256_cases import ROW_TAILS, TILE_ROWS

WORD = 32
ROUTE_OPTS = (("mask_wide", 2), ("mask_tile", 0))
# name -> (engine options, the MFMA shape `last_mfma_shape` must report): the four kernels launch_mfma_scan has a masked form of
VARIANTS = {
    "t128": ((("mfma_tile", 128),), 32),
    "t256m16": ((("mfma_tile", 256), ("mfma_shape", 16)), 16),
    "t256m32": ((("mfma_tile", 256), ("mfma_shape", 32)), 32),
    "t256bd": ((("mfma_tile", 256), ("mfma_bdirect", 1)), 32),
}
ALL_VARIANTS = tuple(VARIANTS)
LADDER_OPTS = (("mfma_sample_rows", 256), ("mfma_ladder", 4))  # phases of 256, 1024 and the rest of a span of 2048+ rows
SPLITS_OPTS = (("mfma_splits", 3), ("mfma_sample_rows", -1))   # one phase, three row ranges of whole tiles


@dataclass(frozen=True)
class Case:
    name: str
    rows: int
    dim: int
    mask: str
    nq: int = 128
    k: int = 10
    thr: str = "zero"  # "zero", "half", "mixed"
    variants: tuple = ALL_VARIANTS  # "auto" among them: no mfma_tile set, the library's own choice (the 128-query tile on these corpora)
    opts: tuple = ()
    span: str = "tight"  # "tight": (first, last) allowed row; "whole": (0, rows - 1)
    dups: tuple = ()  # (first row, count, query): that many copies of the query from that row on (the flagged-query re-run)
    seed: int = 0

    @property
    def padded(self) -> bool:
        return self.dim % 64 != 0


def variant_opts(case: Case, variant: str) -> tuple:
    return () if variant == "auto" else VARIANTS[variant][0]


def variant_shape(case: Case, variant: str) -> int:
    return 32 if variant == "auto" else VARIANTS[variant][1]  # (auto: the 128-query tile on corpora this small, always 32x32x16)


@functools.lru_cache(maxsize=8)
def _inputs(rows: int, dim: int, nq: int, dups: tuple, seed: int):
    v, _ = make_corpus(rows, dim, seed)
    qs = make_queries(nq, dim, seed + 1)
    if dups:
        first, count, qi = dups
        v[first: first + count] = qs[qi]
    store = v.astype(np.float16)
    return store.astype(np.float32), store, qs


def case_inputs(case: Case):
    """-> (the values the kernels multiply, float32 [rows, dim]; the rows as stored, float16; the queries float32 [nq, dim])"""
    return _inputs(case.rows, case.dim, case.nq, case.dups, case.seed)


@functools.lru_cache(maxsize=8)
def case_mask(case: Case) -> np.ndarray:
    n, kind = case.rows, case.mask
    r = np.arange(n)
    rng = np.random.default_rng(case.seed + 77)
    if kind == "all":
        return np.ones(n, dtype=bool)
    if kind == "none":
        return np.zeros(n, dtype=bool)
    if kind.startswith("one@"):  # a single row: "one@last" or "one@<row>"
        m = np.zeros(n, dtype=bool)
        m[n - 1 if kind == "one@last" else int(kind[4:])] = True
        return m
    if kind == "alt":
        return r % 2 == 0
    if kind == "altword":
        return (r // WORD) % 2 == 1
    if kind in ("group80", "group80c"):  # every other 80-row admission group of the 16x16x32 form empty, its neighbour full -- and the complement
        full = (r // 80) % 2 == 0
        return full if kind == "group80" else ~full
    if kind == "rand50":
        return rng.random(n) < 0.5
    if kind.startswith("range"):  # "range700-1500": rows [700, 1500)
        lo, hi = (int(x) for x in kind[5:].split("-"))
        return (r >= lo) & (r < hi)
    raise ValueError(kind)


def case_words(case: Case, garbage: bool = False) -> np.ndarray:
    """the mask in the library's bit form, uint32 [(rows + 31) // 32]; garbage: the bits at and beyond `rows` in the last word set"""
    n_words = (case.rows + WORD - 1) // WORD
    padded = np.zeros(n_words * WORD, dtype=bool)
    padded[: case.rows] = case_mask(case)
    if garbage:
        padded[case.rows:] = True
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def case_garbage(case: Case) -> bool:
    return case.seed % 2 == 1


def case_span(case: Case):
    flat = np.flatnonzero(case_mask(case))
    if len(flat) == 0:
        return None
    return (0, case.rows - 1) if case.span == "whole" else (int(flat[0]), int(flat[-1]))


def span_rows(case: Case) -> tuple[int, int]:
    """[begin, end) of the rows the filter scans: the span with its begin rounded down to a multiple of 256"""
    first, last = case_span(case)
    return first // 256 * 256, last + 1


def case_thresholds(case: Case) -> np.ndarray:
    from typeagent_py_amd import _native

    pattern = {"zero": [0.0], "half": [0.5], "mixed": [0.0, 0.5, float("nan"), 1.5, 0.52]}[case.thr]
    return np.array([_native.f32_threshold(pattern[i % len(pattern)]) for i in range(case.nq)], dtype=np.float32)


def phase_starts(case: Case) -> list[int]:
    """the corpus row every phase starts at under an explicit mfma_sample_rows (tavb_route.hip::ladder_bounds over the span)"""
    from tests.wide256_cases import ladder_bounds

    begin, end = span_rows(case)
    o = dict(case.opts)
    sample = o.get("mfma_sample_rows", 0)
    assert sample != 0, "stated for an explicit first phase only"
    return [begin + b for b in ladder_bounds(end - begin, max(sample, 0), o.get("mfma_ladder", 4))[:-1]]


def range_starts(case: Case) -> list[int]:
    """the corpus row every row range of a ONE-phase run under a forced mfma_splits starts at (fill_device_params: whole 320-row tiles)"""
    begin, end = span_rows(case)
    splits = dict(case.opts)["mfma_splits"]
    per = -(-(end - begin) // splits)
    per = -(-per // TILE_ROWS) * TILE_ROWS
    return [begin + i * per for i in range(splits) if i * per < end - begin]


# ---- which word and bit of the mask each lane tests (the kernel's admission slow path, restated)
def tile_reads_32(row0: int):
    """32x32x16 form: arrays over (wm 2, mi 5, lane 64, register 16) -> (word index, bit, the corpus row the register holds).  Block (wm, mi) is
    the ONE word (row0 + 160 wm + 32 mi) >> 5; register r = 4 g + j holds row r_off = j + 8 g from the lane's first row, 4 (lane >> 5)."""
    wm, mi, lane, reg = np.meshgrid(np.arange(2), np.arange(5), np.arange(64), np.arange(16), indexing="ij")
    block_row = row0 + 160 * wm + 32 * mi
    r_off = (reg % 4) + 8 * (reg // 4)
    bit = r_off + 4 * (lane >> 5)
    return block_row >> 5, bit, block_row + bit


def tile_reads_16(row0: int):
    """16x16x32 form: arrays over (wm 2, h 2, lane 64, m 5, j 4) -> (first word loaded, words loaded, bit relative to the first word's bit 0,
    the corpus row).  Group (wm, h) starts at row0 + 160 wm + 80 h -- bit 0 (h = 0) or 16 (h = 1) of word W -- and reads W, W + 1, W + 2."""
    wm, h, lane, m, j = np.meshgrid(np.arange(2), np.arange(2), np.arange(64), np.arange(5), np.arange(4), indexing="ij")
    group_row = row0 + 160 * wm + 80 * h
    sh = group_row & 31
    rel = 16 * m + j + 4 * (lane >> 4)
    return group_row >> 5, 3, sh + rel, group_row + rel


def _seed(i: int) -> int:
    return 950_000 + 16 * i


def _table() -> list[Case]:
    out: list[Case] = []

    def add(name, rows, dim, mask, **kw):
        out.append(Case(name, rows, dim, mask, seed=_seed(len(out)) + kw.pop("odd", 0), **kw))

    # queries: 128 and 129 at the library's own choice and forced; 256 / 257 (a query tail of one) on the 256-query tile in all its forms
    for nq, variants in ((128, ("auto", "t128")), (129, ("auto", "t128", "t256m16")), (256, ("auto", *ALL_VARIANTS)), (257, ALL_VARIANTS)):
        add(f"nq{nq}-rand50", 1283, 128, "rand50", nq=nq, k=64, variants=variants)
    # widths: one, two and three K steps, and an odd width through the zero-padded copy of the rows
    for d in (64, 192, 100):
        add(f"width-d{d}", 963, d, "rand50", nq=256, k=64, odd=1)
    # row tails around the 80-row group, the 160-row wave and the tile, behind one full tile; garbage behind the corpus in the last word
    for t in ROW_TAILS:
        if t in (79, 80, 81, 159, 160, 161, 319, 320):
            add(f"tail-r{t}", TILE_ROWS + t, 64, "alt", nq=256, k=256, variants=("t128", "t256m16", "t256m32"), odd=1)
    # masks over 1283 rows = four tiles and three rows; k = 256 at threshold 0: every query returns a fifth of the corpus or every allowed row
    for mk in ("all", "alt", "altword", "group80", "group80c", "rand50"):
        add(f"mask-{mk}", 1283, 64, mk, nq=256, k=256, odd=1 if mk in ("all", "rand50") else 0)
    for pos in (0, 31, 32, 79, 80, 95, 96, 159, 160, 319):  # one bit only, in the SECOND tile
        add(f"mask-one@tile+{pos}", 1283, 64, f"one@{TILE_ROWS + pos}", nq=256, k=10, span="whole", variants=("t128", "t256m16", "t256m32"))
    add("mask-one@last", 1283, 64, "one@last", nq=256, k=10, span="whole", odd=1)
    add("mask-one@last-tight", 1283, 64, "one@last", nq=256, k=10, variants=("t256m16", "t128"))
    # a range that starts at no multiple of 320; the filter starts at row 512, mid-corpus
    add("mask-range700-1500", 2000, 64, "range700-1500", nq=256, k=256)
    add("mask-none-in-span", 1283, 64, "none", nq=256, k=10, span="whole", variants=("t256m16", "t128"))
    # k and thresholds
    for k in (1, 10, 64, 65, 256):
        add(f"k{k}", 1283, 128, "rand50", nq=256, k=k, variants=("t256m16", "t128"))
    add("thr-half", 1283, 128, "rand50", nq=256, k=64, thr="half", variants=("t256m16", "t128"))
    add("thr-mixed", 1283, 128, "rand50", nq=257, k=64, thr="mixed", variants=("t256m16", "t256bd", "t128"), odd=1)
    # several phases (rows 0 / 256 / 1280 of 2600; a span of 2344 rows from row 256: 256 / 512) and forced row ranges: a phase and a row range start mid-mask
    add("ladder-rand50", 2600, 64, "rand50", nq=256, k=64, opts=LADDER_OPTS)
    add("ladder-range300-2600", 2600, 64, "range300-2600", nq=256, k=64, opts=LADDER_OPTS, odd=1)
    add("splits-rand50", 2000, 64, "rand50", nq=256, k=256, opts=SPLITS_OPTS)
    add("splits-range700-1900", 2000, 64, "range700-1900", nq=256, k=64, opts=SPLITS_OPTS)
    # the re-run of flagged queries: 600 copies of query 5 in rows 200 .. 799, every other one allowed -- 300 rows tie at query 5's best score,
    # more than band_max = 256 keys hold
    add("flagged-dups", 1283, 64, "alt", nq=256, k=10, opts=(("band_max", 256),), dups=(200, 600, 5), variants=("t256m16", "t128"))
    return out


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)
RUNS = [(c, v) for c in CASES for v in c.variants]


def oracle_topk_rows(v: np.ndarray, qs: np.ndarray, k: int) -> np.ndarray:
    """[nq, min(k, rows)] rows of every query's top k by the float64 score (ties by row)"""
    s = np.asarray(v, dtype=np.float64) @ np.asarray(qs, dtype=np.float64).T
    return np.argsort(-s, axis=0, kind="stable")[: min(k, s.shape[0])].T


def oracle_tops(case: Case):
    """by the float64 oracle: (every query's unmasked top k rows; every query's top k among the allowed rows, as corpus rows)"""
    v, _, qs = case_inputs(case)
    flat = np.flatnonzero(case_mask(case))
    unmasked = oracle_topk_rows(v, qs, case.k)
    masked = flat[oracle_topk_rows(v[flat], qs, case.k)] if len(flat) else np.zeros((case.nq, 0), dtype=np.int64)
    return unmasked, masked
