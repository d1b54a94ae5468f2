"""Synthetic inputs shared by tests, the golden generator and bench.py.

Recipe = the reference's benchmark script (tools/benchmark_vectorbase.py:80-94 in
/root/reference): one `default_rng(seed)`; corpus = standard_normal((N, D)) as
float32, rows divided by their L2 norm; the query is drawn *after* the corpus
from the same generator and normalised.  (tests/golden/make_golden.py asserts
that this restatement is byte-identical to the reference script's output.)
"""

from __future__ import annotations

import numpy as np


def make_corpus(n: int, d: int, seed: int) -> tuple[np.ndarray, np.ndarray]:
    rng = np.random.default_rng(seed)
    vectors = rng.standard_normal((n, d)).astype(np.float32)
    norms = np.linalg.norm(vectors, axis=1, keepdims=True)
    vectors /= norms
    query = rng.standard_normal(d).astype(np.float32)
    query /= np.linalg.norm(query)
    return vectors, query


def make_queries(count: int, d: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((count, d)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q


def subset_choice(n: int, size: int, seed: int) -> list[int]:
    """tools/benchmark_vectorbase.py:135-136: default_rng(seed).choice(n, size, replace=False).tolist()"""
    return np.random.default_rng(seed).choice(n, size=size, replace=False).tolist()


def explicit_case_arrays(case: dict) -> tuple[np.ndarray, np.ndarray]:
    """(vectors [N, D], query [D]) of an `explicit` golden case (N may be 0)."""
    q = np.asarray(case["query"], dtype=np.float32)
    v = np.asarray(case["vectors"], dtype=np.float32).reshape(-1, q.shape[0])
    return v, q


def make_clustered_corpus(n: int, d: int, seed: int, cluster_rows: int = 100, spread: float = 0.002, n_queries: int = 0):
    """Clustered twin of make_corpus (the host-side restatement of bench.py's `kind="clustered"` recipe, scaled down): n // cluster_rows
    unit centres; row i belongs to cluster (i * 7368787) % n_clusters and is centre + spread * noise / sqrt(d), normalised; every row with
    i % 8 == 5 takes the NEXT cluster's centre as its noise -- those rows of a cluster are exact duplicates of one another.  Queries sit
    next to centres (centre + 0.05 * noise / sqrt(d)): their top hits are one cluster, with scores packed inside ~spread / 10.
    Returns (vectors [n, d] float32, queries [n_queries, d] float32, cluster id of every row, cluster id of every query)."""
    rng = np.random.default_rng(seed)
    n_c = max(1, n // cluster_rows)
    centres = rng.standard_normal((n_c, d)).astype(np.float32)
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    ids = np.arange(n, dtype=np.int64)
    cl = (ids * 7_368_787) % n_c
    v = rng.standard_normal((n, d)).astype(np.float32) * np.float32(spread / np.sqrt(d))
    dup = (ids % 8) == 5
    v[dup] = centres[(cl[dup] + 1) % n_c] * np.float32(spread)
    v += centres[cl]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    qc = rng.choice(n_c, size=n_queries, replace=n_c < n_queries) if n_queries else np.zeros(0, dtype=np.int64)
    q = centres[qc] + np.float32(0.05 / np.sqrt(d)) * rng.standard_normal((n_queries, d)).astype(np.float32)
    if n_queries:
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    return v.astype(np.float32), q.astype(np.float32), cl, qc


ANISO_C = float(np.sqrt(3.0))  # bench.py ANISO_C: |c * mu| over |g|; cosine between two rows ~ c^2 / (1 + c^2) = 0.75


def _aniso_direction(d: int, seed: int) -> np.ndarray:
    mu = np.random.default_rng(seed * 1_000_003 + 999_979).standard_normal(d).astype(np.float32)
    return mu / np.linalg.norm(mu)


def make_aniso_corpus(n: int, d: int, seed: int) -> np.ndarray:
    """Host restatement of bench.py's `kind="aniso"` recipe (not its bytes: bench draws on the device): one unit direction mu per seed;
    row = normalise(g + ANISO_C * sqrt(d) * mu), g standard normal.  Mean pairwise cosine 0.75, so a query of the same distribution
    (`aniso_queries`) scores almost every row near 0.875: thousands of survivors at min_score 0.85 and near-ties at any rank."""
    mu = _aniso_direction(d, seed)
    v = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    v += np.float32(ANISO_C * np.sqrt(d)) * mu
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(np.float32)


def aniso_queries(count: int, d: int, seed: int) -> np.ndarray:
    """`count` unit queries from the distribution of `make_aniso_corpus(.., d, seed)`'s rows (bench.py aniso_queries)."""
    mu = _aniso_direction(d, seed)
    q = np.random.default_rng(seed + 23).standard_normal((count, d)).astype(np.float32)
    q += np.float32(ANISO_C * np.sqrt(d)) * mu
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(np.float32)
