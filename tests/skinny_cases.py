"""The case table of tests/test_gpu_skinny_shapes.py and of its CPU twin tests/test_skinny_cases_host.py: the 32/64-query tile
(`skinny_scan_kernel`, csrc/tavb_mfma_skinny.hip) in all 14 instantiations, at K loops shorter than, equal to and longer than every ring, at
every row tail, under forced row ranges and at every query tail.

Why small corpora and k = 64.  The scores of this tile leave the engine as the tile computed them: nothing rescores them, so a wrong fragment
map, swizzle or wait count is a wrong answer.  A tile is 256 rows (128 in the half-tile variant) x 32 or 64 queries; its epilogue has a 4-row
lane group, an 8-row register group, a 32-row block and a 64-row wave.  With k = 64 (the tile's maximum) over a few hundred rows every query
returns a large share of the corpus and every (row position, query position) class of a tile holds a returned pair: `coverage_holes` states
that as a condition on the INPUTS (computed from the float64 oracle alone) and the CPU twin asserts it for every dense case.

Every run of a case must give the same keys bit for bit: every variant, both K steps, both query tiles and every split count issue the same
MFMA sequence over k in the same order for a given (row, query), and the selection is exact.

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from tests.synth import make_corpus, make_queries
from tests.wide256_cases import oracle_topk_rows, shift_keys  # noqa: F401  (the same rules; re-exported for the two test files)

TILE_ROWS = 256  # BM: rows per tile; a row range is a whole number of them (fill_device_params)
HALF_ROWS = 128  # ... of the half-tile variant (mfma_sched = 6)
CAP = 512  # keys per (workgroup, query) candidate buffer; one that holds more than CAP - rows per tile keys is compacted before the next tile
MAX_K = 64

# the remainders of a row range at every granularity of the epilogue: the 4-row lane group, the 8-row register group, the 32-row block, the
# 64-row wave, the 128-row half tile, the 256-row tile -- one below, on and one above each
ROW_TAILS = (1, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)

# the options that put a small corpus on this tile (after every call: last_tier == 5 and last_shadow == 0)
ROUTE_OPTS = (("direct_group_max_nq", 0), ("small_direct_bytes", 0), ("f32_shadow", 0), ("mfma_min_batch", 1 << 20), ("mfma_min_batch_f32", 1 << 20),
              ("mfma_min_batch_big", 1 << 20), ("mfma_min_batch_big_f32", 1 << 20), ("skinny_min_batch_f16", 1), ("skinny_min_batch_f32", 1))

# last_skinny_kernel = variant * 10000 + bytes per K step * 100 + queries per tile
VARIANT_OF_SCHED = {8: 1, 6: 2, 5: 4}  # mfma_sched -> deep ring, half tiles, register staging (four steps deep)
ALL_KERNELS = {(dt, kid) for dt in ("fp16", "fp32") for kid in (12832, 12864, 6432, 6464, 22832, 32832, 52832)}  # the 14 instantiations


@dataclass(frozen=True)
class Case:
    name: str
    group: str  # "width", "tail", "empty", "compact", "qtail", "kthr", "ladder", "base"
    dtype: str  # of the corpus: "fp16" / "fp32"
    rows: int
    dim: int
    nq: int = 64
    k: int = 64
    splits: tuple = (0,)  # values of mfma_splits the case runs under (0 = the library's choice); the answers must not depend on it
    plant: str = ""  # "blocks": see planted_blocks; "ladder": see planted_ladder
    thr: str = "zero"  # "zero", "fifth" (the 5th-best score of query 0), "mixed" (one threshold per query through search_batch)
    opts: tuple = ()  # further engine options
    base: int = 0  # ordinal base
    seed: int = 0

    @property
    def f32(self) -> bool:
        return self.dtype == "fp32"

    @property
    def row_bytes(self) -> int:
        return self.dim * (4 if self.f32 else 2)

    @property
    def dense(self) -> bool:
        """the cases the coverage condition is stated for: 64 queries, k = 64, threshold 0, more than one tile of rows"""
        return self.group in ("width", "compact", "tail") and self.rows > TILE_ROWS and self.nq == 64 and self.k == MAX_K


# ---- Python mirrors of the library's rules (csrc/tavb_mfma_skinny.hip, csrc/tavb_tile.h)
def skinny_supported(dim: int, k: int, f32: bool) -> bool:
    return (dim * (4 if f32 else 2)) % 64 == 0 and dim > 0 and 1 <= k <= 64


def line_steps(dim: int, f32: bool) -> bool:
    """skinny_line_steps: a row is a whole number of 128-byte lines"""
    return (dim * (4 if f32 else 2)) % 128 == 0


def variant(dim: int, f32: bool, tile: int, sched: int) -> int:
    """skinny_variant"""
    if not line_steps(dim, f32) or sched in (9, 7):
        return 0
    v = VARIANT_OF_SCHED.get(sched, 0)
    if tile != 32:
        v = 0
    steps = dim * (4 if f32 else 2) // 128
    if v >= 3 and steps % v != 0:
        v = 0
    return v


def step_bytes(dim: int, f32: bool, sched: int = 0) -> int:
    return 128 if line_steps(dim, f32) and sched != 9 else 64


def kernel_id(dim: int, f32: bool, tile: int, sched: int = 0) -> int:
    """skinny_kernel_id: what `last_skinny_kernel` must report"""
    return variant(dim, f32, tile, sched) * 10000 + step_bytes(dim, f32, sched) * 100 + tile


def k_steps(case: Case, sched: int = 0) -> int:
    return case.row_bytes // step_bytes(case.dim, case.f32, sched)


def query_tile(nq: int) -> int:
    return 64 if nq > 32 else 32


def row_ranges(rows: int, splits: int) -> list[tuple[int, int]]:
    """the row range of every split under fill_device_params' rounding (ranges are whole 256-row tiles); begin >= end: an empty range"""
    per = (rows + splits - 1) // splits
    per = (per + TILE_ROWS - 1) // TILE_ROWS * TILE_ROWS
    return [(s * per, min(rows, (s + 1) * per)) for s in range(splits)]


@dataclass(frozen=True)
class Run:
    nq: int  # the first nq queries of the case
    sched: int  # mfma_sched
    splits: int  # mfma_splits
    kernel: int  # what last_skinny_kernel must report

    @property
    def what(self) -> str:
        return f"nq {self.nq} mfma_sched {self.sched} mfma_splits {self.splits}"


def runs(case: Case) -> list[Run]:
    """every way a case is run: the whole batch and (of a batch of more than 32) its first 32 queries; a batch of up to 32 on a whole-line
    width again under mfma_sched 8 (deep ring), 6 (half tiles), 5 (register staging: falls back to the ring unless the K steps are a multiple
    of 4) and 9 (64-byte steps); all of it under every mfma_splits of the case"""
    out = []
    f32 = case.f32
    for splits in case.splits:
        sizes = [case.nq] if case.nq <= 32 else [32, case.nq]
        for nq in sizes:
            out.append(Run(nq, 0, splits, kernel_id(case.dim, f32, query_tile(nq), 0)))
        if line_steps(case.dim, f32):
            for sched in (8, 6, 5, 9):
                out.append(Run(sizes[0], sched, splits, kernel_id(case.dim, f32, 32, sched)))
    return out


# ---- the table
TAIL_WIDTHS = (("fp32", 64), ("fp32", 48), ("fp16", 192), ("fp16", 96))  # one whole-line and one half-line width per dtype
WIDTHS = (("fp16", (64, 128, 192, 256, 320, 1536, 3072)),  # whole lines: 1, 2, 3, 4, 5, 24, 48 steps (4, 24, 48: register staging runs)
          ("fp16", (32, 96, 160, 1568)),  # half lines: 1, 3, 5, 49 steps of 64 bytes
          ("fp32", (32, 64, 96, 128, 160, 1536)),  # 1, 2, 3, 4, 5, 48 steps
          ("fp32", (16, 48, 80, 784)))  # 1, 3, 5, 49 steps of 64 bytes

# Seeds.  A dense case needs inputs whose float64 top 64 leave no block class of a tile empty (`coverage_holes`), a qtail case inputs whose
# compared queries have no float64 near tie among their best k + 1 rows; about one seed in two does.  A case's seed is its group's base + what
# is listed here (found by trying 0, 1, 2, ... on the CPU: tests/test_skinny_cases_host.py asserts the outcome, never the search).
SEED_BUMP: dict[str, int] = {
    "width-fp16-d64": 2, "width-fp16-d128": 1, "width-fp16-d320": 1, "width-fp16-d3072": 2, "width-fp16-d32": 2,
    "width-fp16-d1568": 1, "width-fp32-d48": 1, "width-fp32-d128": 1, "tail-fp32-d64-t2-r3": 1, "tail-fp32-d64-t2-r7": 1, "tail-fp32-d64-t2-r32": 1,
    "tail-fp32-d64-t2-r33": 1, "tail-fp32-d64-t2-r128": 1, "tail-fp32-d64-t2-r191": 1, "tail-fp32-d64-t2-r256": 4, "tail-fp32-d48-t2-r4": 1,
    "tail-fp32-d48-t2-r7": 1, "tail-fp32-d48-t2-r32": 1, "tail-fp32-d48-t2-r65": 1, "tail-fp32-d48-t2-r193": 2, "tail-fp32-d48-t2-r255": 1,
    "tail-fp16-d192-t2-r33": 1, "tail-fp16-d192-t2-r63": 1, "tail-fp16-d192-t2-r65": 1, "tail-fp16-d192-t2-r128": 2, "tail-fp16-d192-t2-r192": 3,
    "tail-fp16-d96-t2-r5": 1, "tail-fp16-d96-t2-r63": 1, "tail-fp16-d96-t2-r127": 1, "tail-fp16-d96-t2-r128": 1, "tail-fp16-d96-t2-r191": 1,
    "tail-fp16-d96-t2-r256": 1, "compact-fp16-d192-k64": 1, "qtail-fp32-nq3": 2, "qtail-fp32-nq65": 1, "qtail-fp32-nq96": 1,
    "qtail-fp16-nq33": 1, "qtail-fp16-nq64": 2,
}


def _case(name, group, dtype, rows, dim, seed, **kw) -> Case:
    return Case(name, group, dtype, rows, dim, seed=seed + SEED_BUMP.get(name, 0), **kw)


def _widths():
    return [_case(f"width-{dt}-d{d}", "width", dt, 643, d, 100_000 + 16 * d + (8 if dt == "fp32" else 0)) for dt, dims in WIDTHS for d in dims]


def _tails():
    out = []
    for dt, d in TAIL_WIDTHS:
        for t in (0, 2):
            for r in ROW_TAILS:
                rows = TILE_ROWS * t + r
                # t = 2: also as ONE row range (three tiles walked by one workgroup) and as three
                out.append(_case(f"tail-{dt}-d{d}-t{t}-r{r}", "tail", dt, rows, d, 200_000 + 1000 * d + 16 * rows,
                                 splits=(0,) if t == 0 else (0, 1, 3), plant="blocks"))
    return out


def _empties():
    out = []
    for dt, d in TAIL_WIDTHS:
        # 300 rows are two tiles: under 8 (and 5: no multiple of 8, the last three workgroups of the group of 8 return at once) ranges every
        # range from the third on is empty and writes zero lists; 257 rows under 2: a range of one row
        out.append(_case(f"empty-{dt}-d{d}-rows300", "empty", dt, 300, d, 300_000 + d, splits=(8, 5, 0)))
        out.append(_case(f"empty-{dt}-d{d}-rows257", "empty", dt, 257, d, 310_000 + d, splits=(2, 0)))
    return out


ONE_PHASE = (("mfma_sample_rows", -1),)


def _compacts():
    # one workgroup walks six tiles and admits all 1283 rows per query at threshold 0: its buffers are full (CAP) after the second tile and are
    # compacted to the best k there (half tiles: after the fourth, at CAP keys against the limit of CAP - 128); behind the raised thresholds
    # they do not fill again (`compaction_trace`; a second compaction after a refill would take ~10 000 rows).  mfma_sample_rows = -1: ONE
    # phase -- by default a forced single range of 1024 rows and more is scanned as a seeding tile and the rest behind its thresholds
    # (`phase_bounds`), and nothing would run at threshold 0 past the first tile.  The answer must be that of the library's own row ranges.
    return [_case(f"compact-{dt}-d{d}-k{k}", "compact", dt, 1283, d, 400_000 + 16 * d, k=k, splits=(1, 0), opts=ONE_PHASE)
            for dt, d in TAIL_WIDTHS for k in (64, 1, 33)]


QTAIL_NQ = {"fp32": (3, 31, 32, 33, 63, 64, 65, 96, 129, 200), "fp16": (3, 31, 33, 63, 64)}
QTAIL_DIM = {"fp32": 64, "fp16": 96}
KTHR_WIDTHS = (("fp32", 64), ("fp16", 96))
LADDER_OPTS = (("mfma_sample_rows", 256), ("mfma_ladder", 4))  # three phases over 2563 rows: 0, 256, 1280, 2563

CASES = [
    *_widths(),
    *_tails(),
    *_empties(),
    *_compacts(),
    *[_case(f"qtail-{dt}-nq{nq}", "qtail", dt, 643, QTAIL_DIM[dt], 500_000 + 16 * nq + (8 if dt == "fp32" else 0), nq=nq) for dt in ("fp32", "fp16") for nq in QTAIL_NQ[dt]],
    *[_case(f"kthr-{dt}-k{k}", "kthr", dt, 2563, d, 600_000 + d, k=k) for dt, d in KTHR_WIDTHS for k in (1, 2, 32, 63, 64)],
    *[_case(f"kthr-{dt}-fifth-best", "kthr", dt, 2563, d, 600_000 + d, thr="fifth") for dt, d in KTHR_WIDTHS],
    *[_case(f"kthr-{dt}-mixed-thresholds", "kthr", dt, 2563, d, 600_000 + d, thr="mixed") for dt, d in KTHR_WIDTHS],
    *[_case(f"ladder-{dt}-d{d}", "ladder", dt, 2563, d, 700_000 + d, plant="ladder", opts=LADDER_OPTS) for dt, d in TAIL_WIDTHS],
    _case("base-2^32-2-rows", "base", "fp32", 643, 64, 800_000, base=2**32 - 2 - 643),
]
assert len({c.name for c in CASES}) == len(CASES)


def phase_bounds(rows: int, splits: int, sample_opt: int = 0, growth: int = 4) -> list[int]:
    """Phase boundaries of the threshold ladder for this tile under `splits` row ranges (tavb_route.hip::ladder_bounds with skinny = ladder =
    true); sample_opt / growth = the options mfma_sample_rows (0 = auto, -1 = one phase) / mfma_ladder."""
    bounds = [0]
    auto_sample = min(splits, 64) * 320 * 2
    sample = (sample_opt + 255) // 256 * 256 if sample_opt > 0 else (auto_sample if sample_opt == 0 else 0)
    one_tile_each = splits * 256
    if sample_opt == 0 and 4 * one_tile_each <= rows < 2048000:
        bounds.append(one_tile_each)
    elif sample_opt == 0 and rows >= 2048000 and rows >= 32 * one_tile_each:
        bounds.append(one_tile_each)
        if growth > 0:
            bounds.append(13 * one_tile_each)
    elif sample > 0 and rows >= 8 * sample:
        done = sample
        bounds.append(done)
        while growth > 0 and done * (growth + 1) * 2 <= rows and len(bounds) < 8:
            done += done * growth
            bounds.append(done)
    bounds.append(rows)
    return bounds


def case_phase_bounds(case: Case, splits: int) -> list[int]:
    """the phases of a run of the case under a forced mfma_splits"""
    o = dict(case.opts)
    return phase_bounds(case.rows, splits, o.get("mfma_sample_rows", 0), o.get("mfma_ladder", 4))


def case_ladder_bounds(case: Case) -> list[int]:
    """ladder group: an explicit mfma_sample_rows fixes the phases whatever the row ranges"""
    assert dict(case.opts)["mfma_sample_rows"] > 0
    return case_phase_bounds(case, 1)


def compaction_trace(case: Case, tile_rows: int) -> list[list[tuple[int, int]]]:
    """One workgroup over the whole corpus in one phase at threshold 0, by the float64 oracle: per query the (tile index, keys in the buffer)
    of every compaction.  As the kernel: a tile appends every row scoring above the query's threshold (none at first); a buffer that holds
    more than CAP - tile_rows keys after a tile is cut to its best k and the k-th best becomes the threshold (a later tie loses)."""
    v, _, qs = case_inputs(case)
    s = np.asarray(v, dtype=np.float64) @ np.asarray(qs, dtype=np.float64).T  # [rows, nq]
    out = []
    for q in range(case.nq):
        kept, thr, trace = np.zeros(0), -np.inf, []
        n_tiles = (case.rows + tile_rows - 1) // tile_rows
        for t in range(n_tiles):
            col = s[t * tile_rows: (t + 1) * tile_rows, q]
            kept = np.concatenate([kept, col[col > thr]])
            assert kept.size <= CAP, "a buffer overflowed: keys would be dropped"
            if kept.size > CAP - tile_rows and t + 1 < n_tiles:  # (after the last tile nothing is compacted for: the buffer is sorted)
                trace.append((t, int(kept.size)))
                if kept.size > case.k:
                    kept = np.sort(kept)[::-1][: case.k]
                    thr = kept[-1]
        out.append(trace)
    return out


def planted_blocks(rows: int, nq: int) -> dict[int, int]:
    """query -> the row that holds a copy of it: query 0 the LAST row of the corpus, query 1 + b the last row of the b-th complete 32-row block
    of the last tile"""
    where = {0: rows - 1}
    tile0 = (rows - 1) // TILE_ROWS * TILE_ROWS
    for b in range((rows - tile0) // 32):
        row = tile0 + 32 * b + 31
        if row != rows - 1 and 1 + b < nq:
            where[1 + b] = row
    return where


def planted(case: Case) -> dict[int, int]:
    if case.plant == "blocks":
        return planted_blocks(case.rows, case.nq)
    if case.plant == "ladder":  # a best hit inside the first phase, in the last rows and in the first row behind every inner bound
        where = {0: 5, 1: case.rows - 3}
        for i, edge in enumerate(case_ladder_bounds(case)[1:-1]):
            where[2 + i] = edge
        return where
    return {}


@functools.lru_cache(maxsize=4)
def _inputs(case: Case):
    v, _ = make_corpus(case.rows, case.dim, case.seed)
    qs = make_queries(case.nq, case.dim, case.seed + 1)
    for qi, row in planted(case).items():
        v[row] = qs[qi]
    if case.dtype == "fp16":
        store = v.astype(np.float16)
        return store.astype(np.float32), store, qs
    return v, v, qs


def case_inputs(case: Case):
    """-> (the values the kernel multiplies as float32 [rows, dim]: the fp16-rounded rows of an fp16 corpus; the rows as stored (float16 or
    float32); the queries float32 [nq, dim], which the kernel multiplies unrounded).  Gaussian unit rows and queries (tests/synth.py); a
    planted row is a copy of its query."""
    return _inputs(case)


def coverage_holes(rows: int, topk_rows: np.ndarray, tile_rows: int = TILE_ROWS) -> tuple[list, list]:
    """The classes of a tile that NO returned (row, query) pair falls into, of those the corpus has rows for:
      (row mod tile_rows, query // 32)        -- every row of a tile against every 32-query block, and
      (row mod tile_rows // 32, query mod 64) -- every 32-row block against every query lane of the tile.
    Both lists must be empty for a case to prove what it is there to prove."""
    nq = topk_rows.shape[0]
    nqb = (nq + 31) // 32
    q = np.broadcast_to(np.arange(nq)[:, None], topk_rows.shape)
    seen1 = np.zeros((tile_rows, nqb), dtype=bool)
    seen1[topk_rows % tile_rows, q // 32] = True
    seen2 = np.zeros((tile_rows // 32, 64), dtype=bool)
    seen2[(topk_rows % tile_rows) // 32, q % 64] = True
    have_row = np.zeros(tile_rows, dtype=bool)
    have_row[np.arange(rows) % tile_rows] = True
    have_blk = np.zeros(tile_rows // 32, dtype=bool)
    have_blk[(np.arange(rows) % tile_rows) // 32] = True
    have_q = np.zeros(64, dtype=bool)
    have_q[np.arange(nq) % 64] = True
    holes1 = np.argwhere(~seen1 & have_row[:, None]).tolist()
    holes2 = np.argwhere(~seen2 & have_blk[:, None] & have_q[None, :]).tolist()
    return holes1, holes2


def case_holes(case: Case) -> dict[str, tuple[list, list]]:
    """the hole lists of a dense case for each of its runs: 64 queries on 256-row tiles, the first 32 on 256-row and on 128-row (half) tiles"""
    v, _, qs = case_inputs(case)
    top = oracle_topk_rows(v, qs, case.k)
    return {"64 queries": coverage_holes(case.rows, top), "32 queries": coverage_holes(case.rows, top[:32]),
            "32 queries, half tiles": coverage_holes(case.rows, top[:32], HALF_ROWS)}


def single_queries(case: Case) -> list[int]:
    """qtail: the queries compared with their single lookups: the last three and the first of the last query tile"""
    nq = case.nq
    return sorted({q for q in (nq - 1, nq - 2, nq - 3, (nq - 1) // query_tile(nq) * query_tile(nq)) if 0 <= q < nq})
