"""The table of tests/test_pairs_join_host.py (CPU) and tests/test_gpu_pairs_join.py: corpora for the near-duplicate self-join
(`VectorBase.similarity_join`, tavb_join_pairs) and the numpy twin of its bound.

  * `corpus(dtype, rows, dim)`: tests/lookup_rows_cases.pairs_corpus scaled down -- gaussian unit rows with about 150 planted pairs (exact
    copies and near copies at cosine ~0.9998), some rows in triples.  At min_score 0.97 no two unplanted rows pair: their cosine is
    N(0, 1 / dim), 0.94 is 7.5 sigma at dim 64.
  * `edge_corpus(n, dim, dtype)` + `edge_groups(n)`: n rows at every edge of the join's 128 x 128 tile and of its 32 x 32 MFMA blocks, with
    groups of equal or near-equal rows planted inside one 32-row block, across 32-row blocks of one diagonal tile, across tiles, from tile 0
    to the LAST row of a ragged tail tile, inside the tail, as exact copies and as a triple -- whichever of them fit n rows.
  * `join_delta(stored, dtype, dim)`: the join's bound as csrc/tavb_internal.h pairs_join_delta computes it, in float32.
"""

from __future__ import annotations

import functools

import numpy as np

from tests import lookup_rows_cases as lc

MIN_SCORE = 0.97
EDGE_ROWS = (1, 2, 31, 33, 127, 128, 129, 255, 256, 257, 1000)
JOIN = (("pairs_join_min_rows", 1),)                  # the tests force the route: the default keeps small indexes on the row lookups
OLD = lc.STREAM + (("pairs_join", 0),)                # the other leg: the row lookups, their scores the streaming scan's

# (dtype, rows, dim): the corpora of the equality test; the first two also with `among` and every max_per_row
CORPORA = (("fp16", 1000, 64), ("fp32", 1000, 64), ("fp16", 600, 128), ("fp32", 300, 1536))


def corpus(dtype: str, rows: int = 1000, dim: int = 64) -> np.ndarray:
    return lc.pairs_corpus(dtype, rows, dim, min(150, rows // 4))


def stored(v: np.ndarray, dtype: str) -> np.ndarray:
    """the values the device holds, as float32 (fp16 corpora: rounded through float16)"""
    return v.astype(np.float16).astype(np.float32) if dtype == "fp16" else np.asarray(v, np.float32)


def edge_groups(n: int) -> list[tuple[tuple[int, ...], bool]]:
    """(rows of a group of duplicates, exact copies or near copies) -- the groups whose rows all lie below n, no row in two groups"""
    tail = (n - 1) // 128 * 128
    wanted = [
        ((0, 1), True),                         # the smallest index there is
        ((3, 17), False),                       # inside one 32-row block
        ((8, 9, 10), False),                    # a triple
        ((5, 100), True),                       # across 32-row blocks of one diagonal tile
        ((2, 32), False),                       # the first row of the second block
        ((40, 200), False),                     # across tiles
        ((50, n - 1), True),                    # tile 0 and the LAST row (of a ragged tail tile where n is no multiple of 128)
        ((tail + 1, n - 2), False),             # both in the tail tile
        ((64, 127, 128), True),                 # a triple across the quarter and the tile boundary
    ]
    used: set[int] = set()
    out = []
    for rows, exact in wanted:
        if len(set(rows)) == len(rows) and all(0 <= r < n for r in rows) and list(rows) == sorted(rows) and not used & set(rows):
            used |= set(rows)
            out.append((rows, exact))
    return out


@functools.lru_cache(maxsize=None)
def edge_corpus(n: int, dim: int = 64, dtype: str = "fp16") -> np.ndarray:
    rng = np.random.default_rng(500 + n)
    v = rng.standard_normal((n, dim)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    for rows, exact in edge_groups(n):
        for r in rows[1:]:
            w = v[rows[0]] if exact else v[rows[0]] + 0.02 * rng.standard_normal(dim).astype(np.float32) / np.sqrt(dim)
            v[r] = w / np.linalg.norm(w)
    v = stored(v, dtype)
    v.setflags(write=False)
    return v


def planted_pairs(n: int) -> set[tuple[int, int]]:
    return {(a, b) for rows, _ in edge_groups(n) for x, a in enumerate(rows) for b in rows[x + 1:]}


def join_delta(v: np.ndarray, dtype: str, dim: int) -> np.float32:
    """The bound of tavb_join_pairs over the rows the device holds (`v`: float32, fp16 corpora already rounded): R^2 = max ||x16||^2, E^2 = max
    ||x - x16||^2 -- summed in float64 here and rounded UP to float32, the kernels' float32 maxima differ by their own summation rounding,
    which the 1.0001 factors cover -- then csrc/tavb_internal.h pairs_join_delta in float32."""
    f = np.float32
    x16 = v.astype(np.float16).astype(np.float64)
    r2 = np.nextafter(f((x16 * x16).sum(axis=1).max()), f(np.inf))
    e2 = f(0.0) if dtype == "fp16" else np.nextafter(f(((v.astype(np.float64) - x16) ** 2).sum(axis=1).max()), f(np.inf))
    R, E = np.sqrt(r2, dtype=f), np.sqrt(e2, dtype=f)
    d = f(0.5) * (E * R * f(1.0001) + E * (R + E) * f(1.0001) + f(2.0) * f(dim // 8 + 8) * f(5.9604645e-8) * (R + E) * (R + E)) + f(1.2e-7)
    return f(d) if np.isfinite(d) else f(np.inf)


def join_threshold(min_score: np.float32, delta: np.float32) -> np.float32:
    lo = np.float32(min_score) - np.float32(2.0) * delta
    return np.nextafter(lo, np.float32(-np.inf)) if lo > 0 else np.float32(-np.inf)


def brute_pairs(v: np.ndarray, min_score: float, allowed: np.ndarray | None = None):
    """float64 scores of every pair i < j -> (i, j, score) of those reaching min_score, and the full score matrix"""
    x = v.astype(np.float64)
    s = np.clip((x @ x.T + 1.0) / 2.0, 0.0, 1.0)
    i, j = np.triu_indices(len(v), 1)
    ok = s[i, j] >= min_score
    if allowed is not None:
        ok &= allowed[i] & allowed[j]
    return i[ok], j[ok], s[i, j][ok], s
