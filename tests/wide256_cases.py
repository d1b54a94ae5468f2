"""The case table of tests/test_gpu_wide256_shapes.py and of its CPU twin tests/test_wide256_cases_host.py: the 256-query filter tile
(`mfma_scan_kernel<..., NI = 4>`, csrc/tavb_mfma_wide.hip) at every width, row tail and query tail, in both MFMA shapes.

Why small corpora and k = 256.  Every key that leaves the engine is rescored exactly, so a filter bug shows only as a MISSING row, and only when
the row it mis-scores belongs to some query's true top k.  A tile is 320 rows x 256 queries; its epilogue has a 4-row lane group, a 16-row
fragment, an 80-row half, a 160-row wave and 16-query (16x16x32) or 32-query (32x32x16) fragments.  With k = 256 over a few hundred rows every
query returns a large share of the corpus, and every (row position, query position) class of a tile is hit by a returned pair:
`coverage_holes` states that as a condition on the INPUTS (computed from the float64 oracle alone), the CPU twin asserts it for every dense
case, so a wrong accumulator-to-row mapping in one block class cannot pass unseen.

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests.synth import make_corpus, make_queries

TILE_ROWS = 320  # BM6: rows per tile of the 128/256-query kernel
TILE_QUERIES = 256
CAPW = 1024  # keys per (workgroup, query) candidate buffer; a buffer holding more than CAPW - TILE_ROWS keys is compacted before the next tile

# the remainders of a row range at every granularity of the 16x16x32 epilogue: the 4-row lane group, the 16-row fragment, the 80-row half,
# the 160-row wave, the 320-row tile -- one below, on and one above each
ROW_TAILS = (1, 3, 4, 5, 15, 16, 17, 79, 80, 81, 159, 160, 161, 239, 240, 241, 319, 320)


@dataclass(frozen=True)
class Case:
    name: str
    group: str  # "width", "tail", "compact", "qtail", "kthr", "ladder", "base"
    dtype: str  # of the corpus: "fp16" / "fp32"
    rows: int
    dim: int
    nq: int = 256
    k: int = 256
    splits: tuple = (0,)  # values of mfma_splits the case runs under (0 = the library's choice); the answers must not depend on it
    plant: str = ""  # "halves": queries copied into the last row and the last row of every complete 80-row half; "ladder": see planted_ladder
    thr: str = "zero"  # "zero", "fifth" (the 5th-best score of query 0), "mixed" (one threshold per query through search_batch)
    opts: tuple = ()  # further engine options
    base: int = 0  # ordinal base
    seed: int = 0

    @property
    def padded(self) -> bool:
        """the filter reads a copy of the rows: the fp16 shadow of an fp32 corpus, the zero-padded copy of a width that is no multiple of 64"""
        return self.dtype == "fp32" or self.dim % 64 != 0

    @property
    def dense(self) -> bool:
        """the cases the coverage conditions are stated for (groups 1-3: 256 queries, k = 256, threshold 0)"""
        return self.group in ("width", "tail", "compact")


def _widths():
    out = []
    for d in (64, 128, 192, 320, 960, 1536, 3072, 4096):  # 1, 2, 3, 5, 15, 24, 48, 64 K steps
        out.append(Case(f"width-f16-d{d}", "width", "fp16", 643, d, seed=100 + d))
    for d in (33, 100, 130, 1000):  # zero-padded to 64, 128, 192, 1024
        out.append(Case(f"width-f16-padded-d{d}", "width", "fp16", 643, d, seed=200 + d))
    for d in (64, 80, 192, 1536):  # through the fp16 shadow (80: a multiple of 16, padded to 128)
        out.append(Case(f"width-f32-shadow-d{d}", "width", "fp32", 643, d, seed=300 + d))
    return out


def _tails():
    out = []
    for d in (64, 192):
        for t in (0, 2):
            for r in ROW_TAILS:
                rows = TILE_ROWS * t + r
                # t = 2: also as ONE row range (three tiles walked by one workgroup) and as three.  Ranges are whole tiles, so the two range ends
                # inside the corpus fall on multiples of 320 (a full last tile of a range followed by another range); the remainder r itself
                # is met at the end of the corpus only, in every split
                out.append(Case(f"tail-d{d}-t{t}-r{r}", "tail", "fp16", rows, d, splits=(0,) if t == 0 else (0, 1, 3), plant="halves",
                                seed=1000 + 7 * d + rows))
    return out


LADDER_OPTS = {64: (("mfma_sample_rows", 1536), ("mfma_ladder", 4)), 192: (("mfma_sample_rows", 1280), ("mfma_ladder", 4))}

CASES = [
    *_widths(),
    *_tails(),
    # one workgroup walks five tiles and appends 1283 keys per query at threshold 0: more than CAPW - TILE_ROWS = 704, so the band compaction (compact_buffer<CAPW, true>) runs
    # between tiles; the answer must be that of the library's own row ranges
    *[Case(f"compact-d{d}", "compact", "fp16", 1283, d, splits=(1, 0), seed=2000 + d) for d in (64, 192)],
    *[Case(f"qtail-nq{nq}-k{k}", "qtail", "fp16", 643, 192, nq=nq, k=k, seed=3000) for k in (32, 256) for nq in (65, 129, 143, 255, 256, 257, 513)],
    *[Case(f"kthr-k{k}", "kthr", "fp16", 2563, 320, k=k, seed=4000) for k in (1, 64, 65, 256)],
    Case("kthr-fifth-best", "kthr", "fp16", 2563, 320, k=64, thr="fifth", seed=4000),
    Case("kthr-mixed-thresholds", "kthr", "fp16", 2563, 320, k=64, thr="mixed", seed=4000),
    Case("ladder-d64", "ladder", "fp16", 16_003, 64, plant="ladder", opts=LADDER_OPTS[64], seed=5064),
    Case("ladder-d192", "ladder", "fp16", 12_963, 192, plant="ladder", opts=LADDER_OPTS[192], seed=5192),
    Case("base-2^32-2-rows", "base", "fp16", 643, 192, base=2**32 - 2 - 643, seed=6000),
]
assert len({c.name for c in CASES}) == len(CASES)


def ladder_bounds(rows: int, sample: int, growth: int) -> list[int]:
    """Phase boundaries of the threshold ladder under an explicit mfma_sample_rows > 0 (tavb_route.hip::ladder_bounds)."""
    sample = (sample + 255) // 256 * 256
    bounds = [0]
    if sample > 0 and rows >= 8 * sample:
        done = sample
        bounds.append(done)
        while growth > 0 and done * (growth + 1) * 2 <= rows and len(bounds) < 8:
            done += done * growth
            bounds.append(done)
    bounds.append(rows)
    return bounds


def case_ladder_bounds(case: Case) -> list[int]:
    return _opts_ladder_bounds(case.rows, case.opts)


def _opts_ladder_bounds(rows: int, opts: tuple) -> list[int]:
    o = dict(opts)
    return ladder_bounds(rows, o["mfma_sample_rows"], o["mfma_ladder"])


def planted_halves(rows: int, nq: int) -> dict[int, int]:
    """query -> the row that holds a copy of it: query 0 the LAST row, query 1 + h the last row of the h-th complete 80-row half"""
    where = {0: rows - 1}
    for h in range(rows // 80):
        row = 80 * h + 79
        if row != rows - 1 and 1 + h < nq:
            where[1 + h] = row
    return where


def planted_ladder(rows: int, opts: tuple) -> dict[int, int]:
    """query -> row: a best hit inside the first phase, in the last rows and in the first row behind every phase boundary"""
    where = {0: 5, 1: rows - 3}
    for i, edge in enumerate(_opts_ladder_bounds(rows, opts)[1:-1]):
        where[2 + i] = edge
    return where


def _planted(plant: str, rows: int, nq: int, opts: tuple) -> dict[int, int]:
    if plant == "halves":
        return planted_halves(rows, nq)
    if plant == "ladder":
        return planted_ladder(rows, opts)
    return {}


def planted(case: Case) -> dict[int, int]:
    return _planted(case.plant, case.rows, case.nq, case.opts)


@functools.lru_cache(maxsize=4)
def inputs(case_key: tuple):
    """(dtype, rows, dim, nq, plant, opts, seed) -> (the values the kernels multiply as float32 [rows, dim], the rows as stored (float16 or
    float32), queries float32 [nq, dim]).  Gaussian unit rows and queries (tests/synth.py); a planted row is a copy of its query."""
    dtype, rows, dim, nq, plant, opts, seed = case_key
    v, _ = make_corpus(rows, dim, seed)
    qs = make_queries(nq, dim, seed + 1)
    for qi, row in _planted(plant, rows, nq, opts).items():
        v[row] = qs[qi]
    if dtype == "fp16":
        store = v.astype(np.float16)
        return store.astype(np.float32), store, qs
    return v, v, qs


def case_inputs(case: Case):
    return inputs((case.dtype, case.rows, case.dim, case.nq, case.plant, case.opts, case.seed))


def oracle_topk_rows(v: np.ndarray, qs: np.ndarray, k: int) -> np.ndarray:
    """[nq, min(k, rows)] rows of every query's top k by the float64 score (ties by row); threshold 0 keeps every row"""
    s = np.asarray(v, dtype=np.float64) @ np.asarray(qs, dtype=np.float64).T  # [rows, nq]; the score map is monotone in the dot product
    order = np.argsort(-s, axis=0, kind="stable")
    return order[: min(k, s.shape[0])].T


def coverage_holes(rows: int, topk_rows: np.ndarray) -> tuple[list, list]:
    """The classes of a tile that NO returned (row, query) pair falls into, of those the corpus has rows for:
      (row mod 320, query // 16 mod 16)   -- every row of a tile against every 16-query fragment, and
      (row mod 320 // 16, query mod 256)  -- every 16-row fragment against every query lane of the tile.
    Both lists must be empty for a case to prove what it is there to prove."""
    nq = topk_rows.shape[0]
    q = np.broadcast_to(np.arange(nq)[:, None], topk_rows.shape)
    seen1 = np.zeros((TILE_ROWS, 16), dtype=bool)
    seen1[topk_rows % TILE_ROWS, (q // 16) % 16] = True
    seen2 = np.zeros((TILE_ROWS // 16, TILE_QUERIES), dtype=bool)
    seen2[(topk_rows % TILE_ROWS) // 16, q % TILE_QUERIES] = True
    have_row = np.zeros(TILE_ROWS, dtype=bool)
    have_row[np.arange(rows) % TILE_ROWS] = True
    have_frag = np.zeros(TILE_ROWS // 16, dtype=bool)
    have_frag[(np.arange(rows) % TILE_ROWS) // 16] = True
    have_q16 = np.zeros(16, dtype=bool)
    have_q16[(np.arange(nq) // 16) % 16] = True
    have_q = np.zeros(TILE_QUERIES, dtype=bool)
    have_q[np.arange(nq) % TILE_QUERIES] = True
    holes1 = np.argwhere(~seen1 & have_row[:, None] & have_q16[None, :]).tolist()
    holes2 = np.argwhere(~seen2 & have_frag[:, None] & have_q[None, :]).tolist()
    return holes1, holes2


def shift_keys(keys: np.ndarray, base: int) -> np.ndarray:
    """base-0 keys -> the keys of the same rows with ordinals + base (empty slots stay 0): (score bits << 32) | (0xFFFFFFFF - ordinal)"""
    k = np.ascontiguousarray(keys).view(np.uint64)
    lo = np.uint64(0xFFFFFFFF) - (k & np.uint64(0xFFFFFFFF)) + np.uint64(base)
    out = (k & np.uint64(0xFFFFFFFF00000000)) | (np.uint64(0xFFFFFFFF) - lo)
    return np.where(k == 0, np.uint64(0), out).view(np.int64)
