"""TEST INFRASTRUCTURE -- the case table of the top-k distinct message lookups (`VectorBase.lookup_top_messages_by_embedding(s)`,
tavb_search_top_messages), shared by tests/test_gpu_top_messages.py (the device) and tests/test_top_messages_host.py (its CPU twin, which
pins the table's own claims against the reference's arithmetic).

Semantics under test, per query e, threshold t and K = max_messages: of every row inside the allowed set whose message is not -1 and
whose score is >= t (NaN never passes), best(m) = the best score of message m's rows; the K messages with the highest best, by
(best descending, message ordinal ascending); min(K, messages with a passing row) of them.

Corpora: the smallest shapes at which a piece can go wrong -- 1 row; 63 / 64 / 65 rows around a wave; 257 past the fused selection; 1000
and 4099 rows for several workgroups and a row tail; widths 8 and 384 (vector tier), 1536 (the single-query tier of one query differs
from the batch's) and 6 (rows that are no 16-byte slices: the scalar tier); fp16 and fp32.
Every corpus of 63 rows and more holds one NaN row and one all-zero row (score 0.5).  A case names a corpus, a row -> message map, the
queries of the batch, K, the thresholds and the allowed set; `CASES` shuffles the axes against one another so that every value of every
axis appears, and tests/test_top_messages_host.py asserts that it does."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests.synth import make_corpus, make_queries


@dataclass(frozen=True)
class Corpus:
    rows: int
    dim: int
    dtype: str  # "float16" / "float32"
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-d{self.dim}-{'f16' if self.dtype == 'float16' else 'f32'}"


CORPORA = (
    Corpus(1, 8, "float32", 9801), Corpus(63, 8, "float16", 9802), Corpus(64, 8, "float32", 9803), Corpus(65, 384, "float16", 9804),
    Corpus(257, 1536, "float32", 9805), Corpus(257, 1536, "float16", 9806), Corpus(1000, 384, "float32", 9807), Corpus(1000, 8, "float16", 9808),
    Corpus(4099, 1536, "float16", 9809), Corpus(4099, 384, "float32", 9810), Corpus(257, 6, "float32", 9811), Corpus(65, 6, "float16", 9812),
)
ROWS = (1, 63, 64, 65, 257, 1000, 4099)
WIDTHS = (6, 8, 384, 1536)
MAPS = ("own", "one", "chunks3", "interleaved", "holes", "sparse")
QUERIES = (1, 2, 8, 9)
KS = (1, 10, 256, 257, "n", "n+5")
THRESHOLDS = ("zero", "tenth", "above", "per_query")
ALLOWED = ("none", "random10", "range", "empty", "message_mask")
MAX_QUERIES = 9


def message_map(rows: int, kind: str) -> np.ndarray:
    """int64 [rows].  own: every row its own message; one: all rows one message; chunks3: 3 contiguous chunks per message; interleaved:
    row % M with M about a quarter of the rows (not monotone: a message's chunks lie far apart); holes: chunks3 with every fifth row -1;
    sparse: chunks3's messages at ordinals 7 m + 2 (n_messages is far larger than the number of messages, and most slots stay empty)."""
    r = np.arange(rows, dtype=np.int64)
    if kind == "own":
        return r
    if kind == "one":
        return np.zeros(rows, dtype=np.int64)
    if kind == "chunks3":
        return r // 3
    if kind == "interleaved":
        return r % max(1, rows // 4)
    if kind == "holes":
        return np.where(r % 5 == 4, -1, r // 3)
    if kind == "sparse":
        return (r // 3) * 7 + 2
    raise ValueError(kind)


@dataclass(frozen=True)
class Case:
    corpus: Corpus
    map: str
    nq: int
    k: object  # an int, "n" (= n_messages) or "n+5"
    thresholds: str
    allowed: str

    @property
    def name(self) -> str:
        return f"{self.corpus.name}-{self.map}-q{self.nq}-k{self.k}-{self.thresholds}-{self.allowed}"


def _cases() -> list[Case]:
    # six cases per corpus; every other axis is its values repeated to that length and shuffled (fixed seed), so that the axes run
    # against one another without a pattern and every value appears about equally often
    n = 6 * len(CORPORA)
    rng = np.random.default_rng(9800)

    def axis(values):
        return [values[j] for j in rng.permutation(np.arange(n) % len(values))]

    maps, nqs, ks, thrs, alls = axis(MAPS), axis(QUERIES), axis(KS), axis(THRESHOLDS), axis(ALLOWED)
    out = [Case(CORPORA[i % len(CORPORA)], maps[i], nqs[i], ks[i], thrs[i], alls[i]) for i in range(n)]
    # pairs the shuffle could miss and that each take another path: the single-query tier at 1536 over a row list; nine queries (a second
    # pass) under a mask; K beyond the messages with a per-query threshold sequence; a message mask over a non-monotone map
    big16, big32 = CORPORA[8], CORPORA[4]
    out += [Case(big16, "chunks3", 1, 10, "zero", "random10"), Case(big32, "interleaved", 1, 257, "tenth", "message_mask"),
            Case(big16, "holes", 9, 256, "per_query", "range"), Case(CORPORA[6], "interleaved", 9, "n+5", "per_query", "message_mask"),
            Case(CORPORA[9], "own", 8, "n", "zero", "none"), Case(CORPORA[0], "own", 1, 1, "zero", "none")]
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


CASES = _cases()

# the cases also judged against the reference's arithmetic on the device (expected answer B): one per corpus, the first in the table
B_CASES = [next(c for c in CASES if c.corpus == corpus and c.allowed != "empty" and c.thresholds != "above") for corpus in CORPORA]

_cache: dict = {}


def corpus_arrays(c: Corpus):
    """(rows as handed to the index, rows as the device holds them (fp16 corpora: rounded to fp16), MAX_QUERIES queries), built once."""
    if c not in _cache:
        v, _ = make_corpus(c.rows, c.dim, c.seed)
        if c.rows >= 63:
            v[c.rows // 3] = np.nan
            v[c.rows // 2] = 0.0
        qs = make_queries(MAX_QUERIES, c.dim, c.seed + 50)
        held = v.astype(np.float16).astype(np.float32) if c.dtype == "float16" else v
        _cache[c] = (v, held, qs)
    return _cache[c]


def n_messages(case: Case) -> int:
    return int(message_map(case.corpus.rows, case.map).max()) + 1


def case_k(case: Case) -> int:
    n = n_messages(case)
    return n if case.k == "n" else n + 5 if case.k == "n+5" else int(case.k)


def tenth_threshold(c: Corpus) -> float:
    """A threshold about a tenth of the rows pass for the corpus' first query: the 0.9 quantile of the reference's own scores."""
    _, held, qs = corpus_arrays(c)
    with np.errstate(invalid="ignore"):
        return float(np.nanquantile(vo.scores_full(held, qs[0]), 0.9))


def case_thresholds(case: Case):
    """One float, or a list with one threshold per query."""
    t = tenth_threshold(case.corpus)
    if case.thresholds == "zero":
        return 0.0
    if case.thresholds == "tenth":
        return t
    if case.thresholds == "above":
        return 1.5
    return [(0.0, t, 1.5, 0.5)[i % 4] for i in range(case.nq)]


def threshold_of(case: Case, qi: int) -> float:
    t = case_thresholds(case)
    return t[qi] if isinstance(t, list) else t


def allowed_messages(case: Case) -> np.ndarray:
    """The scope of the "message_mask" cases: every third message ordinal, and two ordinals that name no message."""
    return np.concatenate([np.arange(0, n_messages(case), 3, dtype=np.int64), [-1, n_messages(case) + 3]])


def case_mask(case: Case):
    """bool [rows], or None: the rows the case searches."""
    rows = case.corpus.rows
    if case.allowed == "none":
        return None
    if case.allowed == "random10":
        return np.random.default_rng(case.corpus.seed + 7).random(rows) < 0.1
    if case.allowed == "range":
        m = np.zeros(rows, dtype=bool)
        m[rows // 4: max(rows // 4 + 1, 3 * rows // 4)] = True
        return m
    if case.allowed == "empty":
        return np.zeros(rows, dtype=bool)
    if case.allowed == "message_mask":
        rm = message_map(rows, case.map)
        return np.isin(rm, allowed_messages(case)) & (rm >= 0)
    raise ValueError(case.allowed)


def collapse(rows, scores, row_to_msg: np.ndarray, k: int):
    """Row hits (any order) -> (messages int64 [m], scores float32 [m]): max per message, rows without a message dropped, sorted by
    (-score, message), cut at k (0: no cut).  What expected answer A does to the library's own row hits."""
    rows = np.asarray(rows, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    msgs = np.asarray(row_to_msg, dtype=np.int64)[rows]
    keep = msgs >= 0
    msgs, scores = msgs[keep], scores[keep]
    if msgs.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    uniq, inv = np.unique(msgs, return_inverse=True)
    best = np.full(len(uniq), -np.inf, dtype=np.float32)
    np.maximum.at(best, inv, scores)
    order = np.lexsort((uniq, -best.astype(np.float64)))
    if k:
        order = order[:k]
    return uniq[order], best[order]


def reference_hits(case: Case, qi: int) -> list[tuple[int, float]]:
    """The reference's row hits of query qi with max_hits = rows: `oracle.vectorbase_oracle.lookup` (`lookup_in_subset` over the allowed
    rows under a mask), rows without a message taken out."""
    _, held, qs = corpus_arrays(case.corpus)
    rm = message_map(case.corpus.rows, case.map)
    thr = vo.f32_threshold(threshold_of(case, qi))
    mask = case_mask(case)
    with np.errstate(invalid="ignore"):
        if mask is None:
            hits = vo.lookup(held, qs[qi], case.corpus.rows, thr)
        else:
            hits = vo.lookup_in_subset(held, qs[qi], np.flatnonzero(mask).tolist(), case.corpus.rows, thr)
    return [(r, s) for r, s in hits if rm[r] >= 0]


def expected_b(case: Case, qi: int) -> list[tuple[int, float]]:
    """Expected answer B: the reference's hits -> `oracle.messages_oracle.memory_messages_from_hits` -> the cut at K.  Its order among
    equal scores is the reference's (first seen), not the library's (ascending ordinal): `judge_b` decides near-ties."""
    out = mo.memory_messages_from_hits(reference_hits(case, qi), message_map(case.corpus.rows, case.map))
    k = case_k(case)
    return out[:k] if k else out


def best_per_message(case: Case, qi: int):
    """(float32 reference best score per message ordinal, NaN where the message has no allowed row with a score; the same in float64)
    over the allowed rows: what `judge_b` hands `check_topk_parity` as the score vector and the referee."""
    _, held, qs = corpus_arrays(case.corpus)
    rm = message_map(case.corpus.rows, case.map)
    mask = case_mask(case)
    rows = np.arange(case.corpus.rows) if mask is None else np.flatnonzero(mask)
    rows = rows[rm[rows] >= 0]
    n = n_messages(case)
    best32 = np.full(n, np.nan, dtype=np.float32)
    best64 = np.full(n, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        s32 = vo.scores_full(held[rows], qs[qi]).astype(np.float32) if len(rows) else np.zeros(0, np.float32)
        s64 = vo.scores_f64(held[rows], qs[qi]) if len(rows) else np.zeros(0)
    np.fmax.at(best32, rm[rows], s32)  # (fmax: a NaN row does not hide its message's other rows)
    np.fmax.at(best64, rm[rows], s64)
    return best32, best64


def judge_b(case: Case, qi: int, got_items, got_scores):
    """Judge one query's list against B the way tests/test_gpu_message_scope.py judges its lists: scores within SCORE_TOL of the
    reference's best score of that message, descending, the count min(K, messages with a passing row) up to rows at the threshold, and
    the ordinals B's except among near-ties, which the float64 referee decides (`check_topk_parity` over the best score per message).
    Returns the report."""
    best32, best64 = best_per_message(case, qi)

    def referee(positions):
        return best64[np.asarray(positions, dtype=np.int64)]

    referee.dim = case.corpus.dim
    k = case_k(case)
    thr = float(vo.f32_threshold(threshold_of(case, qi)))
    want = expected_b(case, qi)
    rep = vo.check_topk_parity(best32, got_items, got_scores, k if k else len(best32), thr, referee=referee)
    if not rep.threshold_ambiguous:  # no message sits at the threshold: the count is B's exactly
        assert len(got_items) == len(want), f"{case.name} q{qi}: {len(got_items)} messages, the reference has {len(want)}"
    return rep


# ---- the tie case: 600 identical rows in 600 distinct messages, K = 100, a boundary list of 64 keys -- every key falls into one bucket, so
# the refinement rounds must run (on the message array) and the answer is messages 0 .. 99 in ordinal order, one score
TIE_ROWS, TIE_DIM, TIE_K, TIE_BOUNDARY_KEYS = 600, 8, 100, 64


def tie_corpus():
    row = make_queries(1, TIE_DIM, 9899)[0]
    return np.tile(row, (TIE_ROWS, 1)), make_queries(1, TIE_DIM, 9898)[0]


# ---- the lookup this call exists for: 40 messages of 8 chunks; the query sits next to message 17's chunks, so the best 5 ROWS are all
# message 17's and `lookup_messages_by_embedding(e, 5)` returns one message where a caller asked for five
MOTIVE_MESSAGES, MOTIVE_CHUNKS, MOTIVE_DIM, MOTIVE_NEAR = 40, 8, 64, 17


def motive_corpus():
    rng = np.random.default_rng(9897)
    centres = make_queries(MOTIVE_MESSAGES, MOTIVE_DIM, 9896)
    v = np.repeat(centres, MOTIVE_CHUNKS, axis=0) + np.float32(0.02) * rng.standard_normal((MOTIVE_MESSAGES * MOTIVE_CHUNKS, MOTIVE_DIM)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    q = centres[MOTIVE_NEAR] + np.float32(0.01) * rng.standard_normal(MOTIVE_DIM).astype(np.float32)
    q /= np.linalg.norm(q)
    return v.astype(np.float32), q.astype(np.float32), np.repeat(np.arange(MOTIVE_MESSAGES, dtype=np.int64), MOTIVE_CHUNKS)
