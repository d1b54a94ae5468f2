"""The case table of tests/test_gpu_scoped_wide.py and of its CPU twin tests/test_scoped_wide_host.py: scoped batches (one row mask per query)
on the 128/256-query filter tile (`mfma_scan_scoped_kernel`, csrc/tavb_mfma_wide.hip) followed by exact rescoring -- `tavb_search_scoped_wide`.

What the cases are for.  The route ends in the rescoring, so its answers must EQUAL the row-list route's (`tavb_search_scoped_batch`: ordinals,
float32 score bits, counts).  The filter admits a row for a query only where the query's bit is set in the membership planes, so a plane of the
wrong 32-query block, the wrong 16-bit half, the wrong row of a row pair or a stale phase offset shows as a missing row (a row admitted for a
query whose scope does not hold it shows too: the rescoring never sees a scope).  The corpora are those of tests/masked_wide_cases.py, 640 - 2600
rows, at which the library's own choice is the 128-query tile; the 256-query tile in its three forms is FORCED with `mfma_tile = 256`
(`masked_wide_cases.VARIANTS`) and `last_mfma_shape` says what ran.

Scope families: every one of tests/scoped_batch_cases.py, plus four of this table's own -- "mod32" / "mod16" (query q holds the rows with row %
32 == q % 32, or % 16: the scopes of the queries of one 32-block and of one 16-fragment all differ, and a query's rows sit at one bit position of
every mask word), and "single" / "single7" (query q holds ONE row of the second tile, row 320 + q or 320 + 7 q % 320: with 320 queries every row
position of a tile is some query's only row).

`plane_reads_32` / `plane_reads_16` restate which plane block, word and bit every (wave, block or 80-row group, lane, register) of a tile tests,
in both MFMA shapes; the CPU twin checks them against the row and the query each accumulator register holds.

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests import masked_wide_cases as mw
from tests import scoped_batch_cases as sb
from tests.synth import make_corpus, make_queries
from tests.wide256_cases import TILE_ROWS

ROUTE_OPTS = (("scope_wide", 2), ("scope_tile", 0))
VARIANTS = mw.VARIANTS
ALL_VARIANTS = mw.ALL_VARIANTS
LADDER_OPTS = mw.LADDER_OPTS
SPLITS_OPTS = mw.SPLITS_OPTS
WAVE_OPTS = (("scope_wave_bytes", 1),)  # one query tile per wave
OWN_FAMILIES = ("mod32", "mod16", "single", "single7")
FAMILIES = (*sb.FAMILIES, *OWN_FAMILIES)
ROW_TAILS = (79, 80, 81, 159, 160, 161, 319, 320)


@dataclass(frozen=True)
class Case:
    name: str
    rows: int
    dim: int
    family: str
    nq: int = 256
    k: int = 10
    thr: str = "zero"  # "zero", "half", "mixed" (masked_wide_cases.case_thresholds)
    variants: tuple = ALL_VARIANTS
    opts: tuple = ()
    first: int = 0  # rows below it are cleared from every scope: the span begins there
    dups: tuple = ()  # (first row, count, query): that many copies of the query from that row on, every other one in that query's scope
    seed: int = 0


def variant_opts(variant: str) -> tuple:
    return VARIANTS[variant][0]


def variant_shape(variant: str) -> int:
    return VARIANTS[variant][1]


def variant_tile(variant: str) -> int:
    return dict(VARIANTS[variant][0])["mfma_tile"]


def case_inputs(case: Case):
    """-> (the values the kernels multiply, float32 [rows, dim]; the rows as stored, float16; the queries float32 [nq, dim])"""
    return mw._inputs(case.rows, case.dim, case.nq, case.dups, case.seed)


@functools.lru_cache(maxsize=4)
def case_scopes(case: Case) -> tuple:
    """one bool [rows] array per query"""
    n, nq, r = case.rows, case.nq, np.arange(case.rows)
    if case.family == "mod32":
        out = [r % 32 == q % 32 for q in range(nq)]
    elif case.family == "mod16":
        out = [r % 16 == q % 16 for q in range(nq)]
    elif case.family in ("single", "single7"):
        step = 7 if case.family == "single7" else 1
        out = [r == TILE_ROWS + (step * q) % TILE_ROWS for q in range(nq)]
    else:
        out = [np.array(s) for s in sb.case_scopes(case)]
    if case.first:
        out = [s & (r >= case.first) for s in out]
    if case.dups:  # every other copy, and whatever else the scope held outside the copies
        lo, count, qi = case.dups
        s = out[qi].copy()
        s[lo: lo + count] = (r[lo: lo + count] - lo) % 2 == 0
        out[qi] = s
    return tuple(out)


def case_garbage(case: Case) -> bool:
    """cases that hand the library masks whose last word has ones behind the corpus"""
    return case.seed % 2 == 1


def scope_words(scope: np.ndarray, garbage: bool = False) -> np.ndarray:
    """a scope in the library's bit form, uint32 [(rows + 31) // 32]"""
    n = len(scope)
    padded = np.zeros((n + 31) // 32 * 32, dtype=bool)
    padded[:n] = scope
    if garbage:
        padded[n:] = True
    return np.packbits(padded, bitorder="little").view("<u4").copy()


def union_span(scopes):
    rows = np.flatnonzero(np.logical_or.reduce(scopes))
    return (int(rows[0]), int(rows[-1])) if len(rows) else None


def case_thresholds(case: Case) -> np.ndarray:
    return mw.case_thresholds(case)


def waves(case: Case, variant: str) -> int:
    """waves of query tiles the route makes: one, unless the case sets scope_wave_bytes = 1 (one tile per wave: 256 queries then, or, where
    not even a 256-query tile fits and the tile is forced to 128, 128)"""
    if dict(case.opts).get("scope_wave_bytes", 64 << 20) >= 64 << 20:
        return 1
    tile = variant_tile(variant)
    return -(-case.nq // tile)


# ---- which plane block, word and bit each lane tests (the kernel's admission slow path, restated)
def plane_reads_32(row0: int, qtile: int, tile: int):
    """32x32x16 form of the `tile`-query tile (128 or 256): arrays over (wm 2, wn 2, mi 5, ni tile / 64, lane 64, register 16) -> (plane block,
    word = row relative to the launch's first row, bit).  Block (wm, mi) x (wn, ni) loads the 32 words from row0 + 160 wm + 32 mi on of plane
    block (qtile * tile + wn * tile / 2) / 32 + ni; register r = 4 g + j is ANDed with word 8 g + j in lanes 0 - 31 and word 8 g + j + 4 in
    lanes 32 - 63, bit = lane & 31."""
    ni_n = tile // 64
    wm, wn, mi, ni, lane, reg = np.meshgrid(np.arange(2), np.arange(2), np.arange(5), np.arange(ni_n), np.arange(64), np.arange(16), indexing="ij")
    block = (qtile * tile + wn * (tile // 2)) // 32 + ni
    g, j = reg // 4, reg % 4
    word = row0 + 160 * wm + 32 * mi + 8 * g + j + 4 * (lane >> 5)
    return block, word, lane & 31


def plane_reads_16(row0: int, qtile: int):
    """16x16x32 form (the 256-query tile): arrays over (wm 2, wn 2, h 2, n 8, lane 64, m 5, j 4) -> (plane block, word, bit).  Group (wm, h) x
    fragment (wn, n) loads per m the 16 words from row0 + 160 wm + 80 h + 16 m on of plane block (qtile * 256 + wn * 128) / 32 + n / 2; the
    mask of (m, j) takes from word j + 4 g its 16-bit half n & 1 for the lanes 16 g .. 16 g + 15: bit = 16 (n & 1) + (lane & 15), g = lane >> 4."""
    wm, wn, h, n, lane, m, j = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), np.arange(8), np.arange(64), np.arange(5), np.arange(4), indexing="ij")
    block = (qtile * 256 + wn * 128) // 32 + n // 2
    word = row0 + 160 * wm + 80 * h + 16 * m + j + 4 * (lane >> 4)
    return block, word, 16 * (n & 1) + (lane & 15)


def acc_holds_32(row0: int, qtile: int, tile: int):
    """what the accumulators hold, from the MFMA's own result layout (v_mfma_f32_32x32x16: lane l = column l & 31, register r = row (r & 3) + 8
    (r >> 2) + 4 (l >> 5) of the 32 x 32 block): arrays shaped like plane_reads_32's -> (corpus row relative to the launch, padded query)"""
    ni_n = tile // 64
    wm, wn, mi, ni, lane, reg = np.meshgrid(np.arange(2), np.arange(2), np.arange(5), np.arange(ni_n), np.arange(64), np.arange(16), indexing="ij")
    row = row0 + 160 * wm + 32 * mi + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    query = qtile * tile + wn * (tile // 2) + 32 * ni + (lane & 31)
    return row, query


def acc_holds_16(row0: int, qtile: int):
    """v_mfma_f32_16x16x32: lane l = column l & 15, register j = row j + 4 (l >> 4) of the 16 x 16 block; block (m, n) of group (wm, h) x wave
    column wn: rows 160 wm + 80 h + 16 m .., queries 128 wn + 16 n .."""
    wm, wn, h, n, lane, m, j = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), np.arange(8), np.arange(64), np.arange(5), np.arange(4), indexing="ij")
    row = row0 + 160 * wm + 80 * h + 16 * m + j + 4 * (lane >> 4)
    query = qtile * 256 + 128 * wn + 16 * n + (lane & 15)
    return row, query


def _seed(i: int) -> int:
    return 970_000 + 16 * i


def _table() -> list[Case]:
    out: list[Case] = []

    def add(name, rows, dim, family, **kw):
        out.append(Case(name, rows, dim, family, seed=_seed(len(out)) + kw.pop("odd", 0), **kw))

    # batches: 128 and 129 on the 128-query tile (129: a second tile of one query), 256 and 257 (a query tail of one) on all four
    for nq, variants in ((128, ("t128",)), (129, ("t128", "t256m16")), (256, ALL_VARIANTS), (257, ALL_VARIANTS)):
        add(f"nq{nq}-random50%", 1283, 128, "random50%", nq=nq, k=64, variants=variants)
    # every family of the scoped batches on every variant; widths 64 / 128 / 192 / 100 (the zero-padded copy) and k rotate
    for i, fam in enumerate(sb.FAMILIES):
        add(f"family-{fam}", (1283, 963, 640)[i % 3], (64, 128, 192, 100)[i % 4], fam, nq=(256, 257)[i % 2], k=(10, 64, 256)[i % 3], odd=i % 2)
    # scopes that differ between the queries of one 32-block / one 16-fragment; one row per query at every position of the second tile
    add("mod32", 1283, 64, "mod32", nq=257, k=64, odd=1)
    add("mod16", 1283, 64, "mod16", nq=256, k=256)
    add("single", 1283, 64, "single", nq=320, k=10)
    add("single7", 1283, 64, "single7", nq=320, k=10, odd=1)
    # row tails around the 80-row group, the 160-row wave and the tile, behind one full tile; garbage behind the corpus in the masks' last words
    for t in ROW_TAILS:
        add(f"tail-r{t}", TILE_ROWS + t, 64, ("random50%", "mod16", "disjoint")[t % 3], nq=256, k=256, variants=("t128", "t256m16", "t256m32"), odd=1)
    # k and thresholds
    for k in (1, 10, 64, 65, 256):
        add(f"k{k}", 1283, 128, "random50%", nq=256, k=k, variants=("t256m16", "t128"))
    add("thr-half", 1283, 128, "nested", nq=256, k=64, thr="half", variants=("t256m16", "t128"))
    add("thr-mixed", 1283, 128, "random50%", nq=257, k=64, thr="mixed", odd=1)
    # two phases over a span that begins mid-corpus (they start at rows 256 and 512 of 2600): with disjoint scopes -- row r belongs to query r % 256 --
    # cleared below row 300, queries 0 .. 43 have no row in the first phase; forced row ranges in one phase
    add("ladder-disjoint", 2600, 64, "disjoint", nq=256, k=10, opts=LADDER_OPTS, first=300)
    add("ladder-random50%", 2600, 64, "random50%", nq=257, k=64, opts=LADDER_OPTS, first=300, odd=1)
    add("splits-random50%", 2000, 64, "random50%", nq=256, k=256, opts=SPLITS_OPTS)
    add("splits-mod32", 2000, 64, "mod32", nq=256, k=64, opts=SPLITS_OPTS, first=700)
    # the re-run of flagged queries: 600 copies of query 5 in rows 200 .. 799, every other one in query 5's scope -- 300 rows tie at its best
    # score, more than band_max = 256 keys hold; the other queries keep their random scopes
    add("flagged-dups", 1283, 64, "random50%", nq=256, k=10, opts=(("band_max", 256),), dups=(200, 600, 5), variants=("t256m16", "t128"))
    # more queries than one wave of planes holds: one tile per wave; the flagged query in a later wave
    add("waves-random50%", 1283, 64, "random50%", nq=513, k=64, opts=WAVE_OPTS, odd=1)
    add("waves-flagged", 1283, 64, "random50%", nq=385, k=10, opts=(*WAVE_OPTS, ("band_max", 256)), dups=(200, 600, 300), variants=("t256m16", "t128"))
    return out


CASES = _table()
assert len({c.name for c in CASES}) == len(CASES)
RUNS = [(c, v) for c in CASES for v in c.variants]


def oracle_topk_rows(v: np.ndarray, q: np.ndarray, k: int) -> np.ndarray:
    """rows of one query's top k by the float64 score (ties by row)"""
    s = np.asarray(v, dtype=np.float64) @ np.asarray(q, dtype=np.float64)
    return np.argsort(-s, kind="stable")[: min(k, len(s))]
