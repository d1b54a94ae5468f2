"""The table of tests/test_lookup_rows_host.py (CPU, a host-only index) and tests/test_gpu_lookup_rows.py: corpora with planted structure, the
rows asked for, max_hits, min_score and -- on the GPU -- the options that pin a route and the getters that prove it.

A corpus is gaussian unit rows with, planted at fixed ordinals:
  * duplicate groups of 2 and 5 exact copies;
  * one group of `big` = k_top + 3 exact copies: for its highest-ordinal member more than k_top equal rows of lower ordinal tie with the row
    itself, so the k_top + 1 list does NOT hold the row (nothing is dropped, the first k_top are kept);
  * a zero row (it scores 0.5 against every row, itself included);
  * one row of norm 3 with a unit copy of its direction before and behind it: its own score clips to 1.0 and ties with both copies.
A min_score of 0.6 lies above the zero row's own score: asked for the zero row, the lookup returns nothing and drops nothing.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

BIG = 1 << 30
ZERO_ROW, NORM3_ROW, NORM3_BEFORE, NORM3_BEHIND = 5, 40, 7, 90
PAIR = (10, 200)
FIVE = (20, 21, 300, 400, 500)


@dataclass(frozen=True)
class Corpus:
    rows: int
    dim: int
    dtype: str  # "fp32" / "fp16"
    big: int    # size of the large duplicate group (k_top + 3)

    @property
    def key(self) -> str:
        return f"{self.dtype}-{self.rows}x{self.dim}"


SMALL32 = Corpus(700, 64, "fp32", 13)
SMALL16 = Corpus(900, 64, "fp16", 13)
ODD32 = Corpus(1100, 100, "fp32", 13)
ODD16 = Corpus(1100, 100, "fp16", 13)
WIDE32 = Corpus(1300, 1536, "fp32", 13)
WIDE16 = Corpus(2600, 1536, "fp16", 259)
CORPORA = (SMALL32, SMALL16, ODD32, ODD16, WIDE32, WIDE16)


def big_group(c: Corpus) -> np.ndarray:
    """ordinals of the large duplicate group, ascending; the last one is the member whose own key is not in its list"""
    return np.arange(c.big, dtype=np.int64) * 2 + 101  # odd ordinals from 101 on (clear of the other planted rows)


@functools.lru_cache(maxsize=None)
def vectors(c: Corpus) -> np.ndarray:
    """float32 [rows, dim]: the values the kernels multiply (fp16 corpora: already rounded through float16)"""
    rng = np.random.default_rng(1000 + c.rows + c.dim)
    v = rng.standard_normal((c.rows, c.dim)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v[PAIR[1]] = v[PAIR[0]]
    for r in FIVE[1:]:
        v[r] = v[FIVE[0]]
    g = big_group(c)
    assert g[-1] < c.rows
    v[g] = v[g[0]]
    v[ZERO_ROW] = 0.0
    v[NORM3_BEFORE] = v[NORM3_BEHIND]
    v[NORM3_ROW] = 3.0 * v[NORM3_BEHIND]
    if c.dtype == "fp16":
        v = v.astype(np.float16).astype(np.float32)
    v.setflags(write=False)
    return v


def special_rows(c: Corpus) -> list[int]:
    g = big_group(c)
    return [int(g[-1]), ZERO_ROW, NORM3_ROW, PAIR[0], PAIR[1], FIVE[0], FIVE[4], int(g[0]), -1, -c.rows, int(g[-1])]


def ordinals(c: Corpus, n: int) -> list[int]:
    """the n rows a case asks for: the planted rows first (a negative ordinal and a repeated one among them), then random ones"""
    head = special_rows(c)
    if n == 1:
        return head[:1]
    if n <= len(head):
        return head[:n]
    rng = np.random.default_rng(c.rows + n)
    return head + rng.integers(-c.rows, c.rows, size=n - len(head)).tolist()


# ---- GPU route forcing (the options of tests/test_gpu_routes.py); every set switches the host-merged one-launch forms off, so that the
# native call and the host route hand the same float32 batch to the same dispatcher
NO_DIRECT = (("small_direct_bytes", 0),)
STREAM = NO_DIRECT + (("skinny_min_batch_f32", BIG), ("skinny_min_batch_f16", BIG), ("mfma_min_batch", BIG), ("mfma_min_batch_f32", BIG), ("mfma_min_batch_big_f32", BIG))
GROUPED = (("direct_group", 2),)  # the grouped launch: the device-resident form on one side, the host-merged form on the other -- the same scan
TILE = NO_DIRECT + (("mfma_min_batch_f32", BIG), ("mfma_min_batch", BIG), ("skinny_min_batch_f32", 2), ("skinny_min_batch_f16", 2))
WIDE128 = NO_DIRECT + (("mfma_tile", 128),)
WIDE256 = NO_DIRECT + (("mfma_tile", 256),)


@dataclass(frozen=True)
class Case:
    name: str
    corpus: Corpus
    n: int
    max_hits: int
    min_score: float = 0.0
    opts: tuple = STREAM
    tiers: tuple = (1, 2, 3)   # allowed "last_tier" after the native call (0: not asserted -- the large-k and sorted routes)
    direct: tuple = (0,)        # allowed "last_direct"
    wave: int = 0               # "rows_query_wave" (0: the default)


CASES = [
    # streaming tiers, every n that fits a few passes, every max_hits
    Case("stream-f32-n1-k1", SMALL32, 1, 1),
    Case("stream-f32-n3-k10", SMALL32, 3, 10),
    Case("stream-f16-n8-k10", SMALL16, 8, 10),
    Case("stream-f16-n9-k63", SMALL16, 9, 63),
    Case("stream-f32-n8-k64", SMALL32, 8, 64),
    # (k + 1 > 64 from 9 queries: the dispatcher's own rule sends the batch to the wide tile whatever "mfma_min_batch" says)
    Case("bigk-wide-f32-n9-k64", SMALL32, 9, 64, 0.0, NO_DIRECT, (4,)),
    Case("stream-odd32-n8-k10", ODD32, 8, 10),
    Case("stream-odd16-n9-k10", ODD16, 9, 10),
    Case("stream-wide32-n3-k10", WIDE32, 3, 10),
    Case("stream-wide16-n8-k255", WIDE16, 8, 255),
    Case("stream-f32-n33-k10-ms06", SMALL32, 33, 10, 0.6),
    Case("stream-wide16-n9-k10-ms06", WIDE16, 9, 10, 0.6),
    Case("stream-f16-n33-k10-waves", SMALL16, 33, 10, 0.0, STREAM, (1, 2, 3), (0,), 8),
    # the grouped launch
    Case("grouped-f32-n33-k10", SMALL32, 33, 10, 0.0, GROUPED, (1, 2, 3), (3, 4)),
    Case("grouped-f16-n64-k63", SMALL16, 64, 63, 0.0, GROUPED, (1, 2, 3), (3, 4)),
    # the 32/64-query tile
    Case("tile32-f32-n9-k10", WIDE32, 9, 10, 0.0, TILE, (5,)),
    Case("tile32-f16-n33-k10", WIDE16, 33, 10, 0.0, TILE, (5,)),
    Case("tile64-f16-n64-k63", WIDE16, 64, 63, 0.0, TILE, (5,)),
    Case("tile64-f32-n65-k10", SMALL32, 65, 10, 0.0, TILE, (5,)),
    # the wide tile in both query-tile widths; k + 1 on both sides of the tile's 64 and of the 256 / 257 hand-over
    Case("wide128-f16-n128-k10", WIDE16, 128, 10, 0.0, WIDE128, (4,)),
    Case("wide256-f16-n257-k10", WIDE16, 257, 10, 0.0, WIDE256, (4,)),
    Case("wide128-f16-n65-k64", WIDE16, 65, 64, 0.0, WIDE128, (4,)),
    Case("wide256-f16-n257-k255", WIDE16, 257, 255, 0.0, WIDE256, (4,)),
    Case("wide-f32-n128-k10", WIDE32, 128, 10, 0.0, NO_DIRECT, (4,)),
    # k + 1 = 257: the device top-k
    Case("topk-f16-n9-k256", WIDE16, 9, 256, 0.0, STREAM, (0,)),
    Case("topk-f32-n33-k256", SMALL32, 33, 256, 0.0, STREAM, (0,)),
    Case("topk-f16-n9-k256-ms06", WIDE16, 9, 256, 0.6, STREAM, (0,)),
    # every survivor
    Case("all-f32-n9", SMALL32, 9, 0, 0.0, STREAM, (0,)),
    Case("all-f16-n33-ms06", SMALL16, 33, 0, 0.6, STREAM, (0,)),
    Case("all-odd16-n3-waves", ODD16, 3, 0, 0.55, STREAM, (0,), (0,), 2),
]

# ---- ordinal edge cases of the class method (CPU and GPU): (name, ordinals, what is expected)
EDGE_CASES = (
    ("negative", [-1, -3], "wrap"),
    ("duplicate-ordinal", [12, 12, 12], "twice"),
    ("out-of-range", [3, 10**6], "IndexError"),
    ("out-of-range-negative", [-(10**6)], "IndexError"),
    ("empty", [], "empty"),
    ("int", 17, "one"),
    ("numpy-array", np.array([4, 8], dtype=np.int32), "wrap"),
)

REQUIRED = frozenset(
    ["self-in-list", "self-not-in-list-duplicates", "zero-row", "norm3-row", "self-below-min-score", "negative", "duplicate-ordinal", "fp16", "fp32",
     "width-64", "width-100", "width-1536", "k+1=64", "k+1=65", "k+1=256", "k+1=257", "every-survivor", "waves", "min-score",
     "route-stream", "route-grouped", "route-tile", "route-wide128", "route-wide256", "route-topk", "route-sorted"]
    + [f"n-{n}" for n in (1, 3, 8, 9, 33, 64, 65, 128, 257)]
    + [f"max_hits-{k}" for k in (1, 10, 63, 64, 255, 256, 0)])


def branches(case: Case) -> set[str]:
    c = case.corpus
    asked = ordinals(c, case.n)
    wrapped = [o + c.rows if o < 0 else o for o in asked]
    out = {c.dtype, f"width-{c.dim}", f"n-{case.n}", f"max_hits-{case.max_hits}", "self-in-list"}
    g = big_group(c)
    if int(g[-1]) in wrapped and 1 <= case.max_hits <= c.big - 3 and case.min_score <= 0.5:
        out.add("self-not-in-list-duplicates")
    if ZERO_ROW in wrapped:
        out.add("zero-row")
        if case.min_score > 0.5:
            out.add("self-below-min-score")
    if NORM3_ROW in wrapped:
        out.add("norm3-row")
    if any(o < 0 for o in asked):
        out.add("negative")
    if len(set(wrapped)) < len(wrapped):
        out.add("duplicate-ordinal")
    if case.max_hits:
        out.add(f"k+1={case.max_hits + 1}")
    else:
        out.update(("every-survivor", "route-sorted"))
    if case.wave and case.wave < case.n:
        out.add("waves")
    if case.min_score > 0:
        out.add("min-score")
    if case.max_hits >= 256:
        out.add("route-topk")
    elif case.max_hits:
        out.add({STREAM: "route-stream", GROUPED: "route-grouped", TILE: "route-tile", WIDE128: "route-wide128", WIDE256: "route-wide256", NO_DIRECT: "route-wide128"}[case.opts])
    return out


# ---- near_duplicate_pairs: a 2000-row corpus with about 150 planted pairs (exact copies and near copies), some rows in triples
@functools.lru_cache(maxsize=None)
def pairs_corpus(dtype: str = "fp32", rows: int = 2000, dim: int = 64, n_pairs: int = 150):
    rng = np.random.default_rng(77)
    v = rng.standard_normal((rows, dim)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    picks = rng.permutation(rows)[: 2 * n_pairs].reshape(n_pairs, 2)
    for t, (a, b) in enumerate(picks.tolist()):
        if t % 3 == 0:
            v[b] = v[a]  # an exact copy
        else:
            w = v[a] + 0.02 * rng.standard_normal(dim).astype(np.float32) / np.sqrt(dim)
            v[b] = w / np.linalg.norm(w)
    for a, b in picks[:20].tolist():  # triples: a third near copy
        c = int(rng.integers(0, rows))
        w = v[a] + 0.02 * rng.standard_normal(dim).astype(np.float32) / np.sqrt(dim)
        v[c] = w / np.linalg.norm(w)
    if dtype == "fp16":
        v = v.astype(np.float16).astype(np.float32)
    v.setflags(write=False)
    return v


def among_mask(rows: int) -> np.ndarray:
    rng = np.random.default_rng(78)
    return rng.random(rows) < 0.6


def definition_pairs(lookup_all, n: int, min_score: float, max_per_row: int, allowed: np.ndarray | None):
    """The host route of near_duplicate_pairs, this loop is the definition: for i in rows, the top max_per_row among rows j > i.
    `lookup_all(i)` -> every row scoring at least min_score against row i as (ordinals, scores), best first, ties by ascending ordinal."""
    out = []
    for i in range(n):
        if allowed is not None and not allowed[i]:
            continue
        js, ss = lookup_all(i)
        kept = [(int(j), float(s)) for j, s in zip(js, ss) if j > i and (allowed is None or allowed[j])][:max_per_row]
        out.extend((i, j, s) for j, s in kept)
    return out
