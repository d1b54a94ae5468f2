"""TEST INFRASTRUCTURE -- the case table of the scoped batches (one row mask per query), shared by tests/test_gpu_scoped_batch.py (the
device) and tests/test_scoped_batch_host.py (its CPU twin, which pins the table's own claims).

A case = a corpus (width, dtype), a row count, a batch size, a max_hits, a family of scopes and a kind of thresholds.  The PASS SHAPE of a
case is (queries, max_hits): it decides how the batch is cut into passes (eight queries per pass, four from max_hits 65 on; a trailing pass
of fewer) and which list depth the kernels keep.  Every scope family runs at every pass shape; corpora and row counts rotate through the
cases so that every corpus meets every row count, every batch size and every max_hits.

`member_bytes` restates `scope_member_kernel` in numpy: bit j of byte p = mask j holds row rows[p]."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

ROWS = (1, 31, 32, 33, 257, 1000, 4099)  # mask-word tails (31 / 32 / 33), the 256-row chunk tail (257), several workgroups (4099)
BATCHES = (1, 2, 3, 5, 8, 9, 17)  # partial passes, a full pass, a trailing pass of one (9 = 8 + 1, 17 = 8 + 8 + 1; at max_hits 65+: 5 = 4 + 1)
MAX_HITS = (1, 10, 64, 65, 256)  # 65 switches to four queries per pass and the 256-deep lists
FAMILIES = ("identical", "disjoint", "nested", "random1%", "random50%", "one_empty", "first_row", "last_row", "all_rows", "all_empty")
THR_CYCLE = (0.0, 0.5, 0.45, 0.55, 1.5, 0.4, None)  # per-query thresholds repeat with the query's index (1.5: nothing passes)


@dataclass(frozen=True)
class Corpus:
    name: str
    dim: int
    dtype: str  # "float32" / "float16"
    tier: int  # the streaming tier a pass of the scoped scan lands on: 2 = vector, 3 = scalar
    seed: int


CORPORA = (
    Corpus("fp32-d8", 8, "float32", 2, 9800),       # the vector tier's smallest fp32 width
    Corpus("fp32-d6", 6, "float32", 3, 9810),       # the scalar tier, both dtypes
    Corpus("fp16-d6", 6, "float16", 3, 9820),
    Corpus("fp16-d72", 72, "float16", 2, 9830),     # rows that are no multiple of a wave's 1 KiB
    Corpus("fp16-d1536", 1536, "float16", 2, 9840),  # where a trailing pass of one query would meet tier 1
    Corpus("fp32-d1536", 1536, "float32", 2, 9850),
)
MAX_ROWS = max(ROWS)
MAX_QUERIES = max(BATCHES)


@dataclass(frozen=True)
class Case:
    corpus: Corpus
    rows: int
    nq: int
    max_hits: int
    family: str
    thresholds: str  # "uniform" / "per_query"
    as_handles: bool  # the scopes are handed over as RowMask handles (else as the bool arrays themselves)

    @property
    def name(self) -> str:
        return f"{self.corpus.name}-r{self.rows}-q{self.nq}-k{self.max_hits}-{self.family}-{self.thresholds}{'' if self.as_handles else '-raw'}"

    @property
    def seed(self) -> int:
        return 9900 + 7 * FAMILIES.index(self.family) + 131 * self.rows + 17 * self.nq + self.max_hits


def _cases() -> tuple[Case, ...]:
    out = []
    i = 0
    for k in MAX_HITS:
        for nq in BATCHES:
            for family in FAMILIES:
                # i runs over 350 cases: corpus, row count, thresholds and the form of the scopes advance with every case and slip by one
                # every 7 or 10 cases, so that each of them meets every value of the others and of (nq, max_hits, family) -- the host test
                # counts the pairs
                out.append(Case(CORPORA[(i + i // 7) % len(CORPORA)], ROWS[(i + i // 10) % len(ROWS)], nq, k, family,
                                "per_query" if (i + i // 10) % 3 == 0 else "uniform", (i + i // 10) % 5 != 0))
                i += 1
    return tuple(out)


CASES = _cases()
# one more, on an adopted device corpus whose ordinals start at ORDINAL_BASE
ORDINAL_BASE = 1_000_003
ADOPTED = Case(CORPORA[3], 1000, 9, 10, "nested", "per_query", True)


def passes(nq: int, max_hits: int) -> list[int]:
    """The queries of every pass of a native scoped batch."""
    per = 4 if max_hits > 64 else 8
    return [min(per, nq - q0) for q0 in range(0, nq, per)]


def case_thresholds(case: Case):
    """min_score as the caller passes it: one value, or a list with one per query."""
    return [THR_CYCLE[i % len(THR_CYCLE)] for i in range(case.nq)] if case.thresholds == "per_query" else 0.0


def case_scopes(case: Case) -> list[np.ndarray]:
    """One bool [rows] array per query.  Queries that share a scope share the array OBJECT (the class resolves an object once, so they
    share a handle): "identical" is one object for all, "one_empty" one full mask for all but the query in the middle."""
    n, nq = case.rows, case.nq
    rng = np.random.default_rng(case.seed)
    fam = case.family
    if fam == "identical":
        m = rng.random(n) < 0.5
        return [m] * nq
    if fam == "disjoint":  # row r belongs to query r % nq
        return [np.arange(n) % nq == q for q in range(nq)]
    if fam == "nested":  # scope q holds scope q - 1
        u = rng.random(n)
        return [u < (q + 1) / (nq + 1) for q in range(nq)]
    if fam in ("random1%", "random50%"):
        p = 0.01 if fam == "random1%" else 0.5
        return [rng.random(n) < p for _ in range(nq)]
    if fam == "one_empty":  # one empty scope among full ones
        full = np.ones(n, dtype=bool)
        return [np.zeros(n, dtype=bool) if q == nq // 2 else full for q in range(nq)]
    if fam in ("first_row", "last_row"):  # one scope of a single row, at an end of the corpus, among random ones
        out = [rng.random(n) < 0.5 for _ in range(nq)]
        only = np.zeros(n, dtype=bool)
        only[0 if fam == "first_row" else n - 1] = True
        out[nq // 2] = only
        return out
    if fam == "all_rows":  # every scope all rows, each its own object: the union is the corpus and every byte has every bit
        return [np.ones(n, dtype=bool) for _ in range(nq)]
    if fam == "all_empty":
        return [np.zeros(n, dtype=bool) for _ in range(nq)]
    raise ValueError(fam)


def expect_native(scopes: list[np.ndarray]) -> bool:
    """Whether the class hands the case to the native scoped call: at least two distinct scope objects, and something to search."""
    return len({id(s) for s in scopes}) > 1 and any(s.any() for s in scopes)


def member_bytes(masks: list[np.ndarray], rows: np.ndarray) -> np.ndarray:
    """`scope_member_kernel` in numpy: masks = up to 8 bool arrays over the corpus, rows = a row list -> uint8 [len(rows)]."""
    assert 1 <= len(masks) <= 8
    out = np.zeros(len(rows), dtype=np.uint8)
    for j, m in enumerate(masks):
        out |= (m[rows].astype(np.uint8) << j).astype(np.uint8)
    return out
