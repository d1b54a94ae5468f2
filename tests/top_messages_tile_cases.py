"""TEST INFRASTRUCTURE -- the case table of the top-messages lookups on the 32/64-query MFMA tile (tavb_search_top_messages_tile,
engine option "top_messages_tile"), shared by tests/test_gpu_top_messages_tile.py (the device) and tests/test_top_messages_tile_host.py
(its CPU twin, which pins the table's own claims against the reference's arithmetic).

Semantics are tests/top_messages_cases.py's.  What differs is the kernel, so the shapes are the ones at which THIS kernel can go wrong:
  rows      1, 31, 32, 33 (the 32-row block of the epilogue, and the map read at a last partial block), 255, 256, 257 (the tile), 513,
            2049 and 4099 (several tiles, row ranges, a row tail);
  widths    fp16: 32 (one 64-byte K step), 64 (one 128-byte step), 96 (three 64-byte steps), 1536; fp32: 16, 32, 48, 384 -- both K-step
            sizes and a multi-step loop for either dtype;
  queries   1, 31, 32, 33, 64, 65, 129: padding queries, both tile widths, two query tiles, a second group of 64;
  maps      every kind of top_messages_cases.MAPS (rows without a message; chunks3's messages straddle blocks, waves, tiles, row ranges);
  K         1, 10, 65, 257, n, n + 5: beyond 64 the tile's list bound would have refused;
  thresholds zero, tenth, above, per_query;
  masks     none, random 50 %, a range that starts mid-word, all-ones, empty.
Every corpus of 255 rows and more holds one NaN row and one all-zero row (score 0.5).  `CASES` cycles the axes against one another
(fixed seed) so that every value of every axis appears; one more case runs with "topk_scores_bytes" at its floor."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oracle import vectorbase_oracle as vo
from tests.synth import make_corpus, make_queries
from tests.top_messages_cases import MAPS, Corpus, collapse, message_map  # noqa: F401  (collapse: re-exported for the GPU suite)

ROWS = (1, 31, 32, 33, 255, 256, 257, 513, 2049, 4099)
WIDTHS_F16 = (32, 64, 96, 1536)
WIDTHS_F32 = (16, 32, 48, 384)
QUERIES = (1, 31, 32, 33, 64, 65, 129)
KS = (1, 10, 65, 257, "n", "n+5")
THRESHOLDS = ("zero", "tenth", "above", "per_query")
MASKS = ("none", "random50", "range", "ones", "empty")
MAX_QUERIES = 129


def _corpora() -> tuple[Corpus, ...]:
    # every row count with two (dtype, width) pairs, the pairs cycling: 20 corpora, every width at least twice
    shapes = [("float16", w) for w in WIDTHS_F16] + [("float32", w) for w in WIDTHS_F32]
    out = []
    for i, rows in enumerate(ROWS):
        for j in range(2):
            dtype, dim = shapes[(2 * i + j * 5) % len(shapes)]
            out.append(Corpus(rows, dim, dtype, 9900 + 2 * i + j))
    return tuple(out)


CORPORA = _corpora()


@dataclass(frozen=True)
class Case:
    corpus: Corpus
    map: str
    nq: int
    k: object  # an int, "n" (= n_messages) or "n+5"
    thresholds: str
    mask: str
    scores_bytes: int = 0  # > 0: "topk_scores_bytes" for this case (groups below 64 queries)

    @property
    def name(self) -> str:
        return f"{self.corpus.name}-{self.map}-q{self.nq}-k{self.k}-{self.thresholds}-{self.mask}" + ("-floor" if self.scores_bytes else "")


def _cases() -> list[Case]:
    n = 6 * len(CORPORA)
    rng = np.random.default_rng(9900)

    def axis(values):
        return [values[j] for j in rng.permutation(np.arange(n) % len(values))]

    maps, nqs, ks, thrs, masks = axis(MAPS), axis(QUERIES), axis(KS), axis(THRESHOLDS), axis(MASKS)
    out = [Case(CORPORA[i % len(CORPORA)], maps[i], nqs[i], ks[i], thrs[i], masks[i]) for i in range(n)]
    big16 = next(c for c in CORPORA if c.rows == 4099 and c.dtype == "float16")
    big32 = next(c for c in CORPORA if c.rows == 4099 and c.dtype == "float32")
    mid = next(c for c in CORPORA if c.rows == 2049)
    small = next(c for c in CORPORA if c.rows == 257)
    # pairs the shuffle could miss, each another path: chunks3 over several row ranges under both tile widths and a mid-word range; 129
    # queries (a second group) with per-query thresholds; threshold 0 (every pair admits) on 64 queries; sub-groups below 64 queries
    out += [Case(big16, "chunks3", 33, 257, "zero", "range"), Case(big32, "chunks3", 32, 65, "tenth", "random50"),
            Case(mid, "holes", 129, "n", "per_query", "none"), Case(big32, "interleaved", 64, "n+5", "zero", "ones"),
            Case(mid, "sparse", 65, 10, "per_query", "random50"), Case(small, "chunks3", 65, 65, "tenth", "none", scores_bytes=4096)]  # 86 messages: groups of 11 queries
    seen, uniq = set(), []
    for c in out:
        if c.name not in seen:
            seen.add(c.name)
            uniq.append(c)
    return uniq


CASES = _cases()

_cache: dict = {}


def corpus_arrays(c: Corpus):
    """(rows as handed to the index, rows as the device holds them (fp16 corpora: rounded to fp16), MAX_QUERIES queries), built once."""
    if c not in _cache:
        v, _ = make_corpus(c.rows, c.dim, c.seed)
        if c.rows >= 255:
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
    key = ("tenth", c)
    if key not in _cache:
        _, held, qs = corpus_arrays(c)
        with np.errstate(invalid="ignore"):
            _cache[key] = float(np.nanquantile(vo.scores_full(held, qs[0]), 0.9))
    return _cache[key]


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


def case_mask(case: Case):
    """bool [rows], or None: the rows the case searches.  range: from row rows // 4 | 5 (mid-word wherever there are that many rows) on."""
    rows = case.corpus.rows
    if case.mask == "none":
        return None
    if case.mask == "random50":
        return np.random.default_rng(case.corpus.seed + 7).random(rows) < 0.5
    if case.mask == "range":
        m = np.zeros(rows, dtype=bool)
        first = min(rows - 1, (rows // 4) | 5)
        m[first: max(first + 1, 3 * rows // 4)] = True
        return m
    if case.mask == "ones":
        return np.ones(rows, dtype=bool)
    if case.mask == "empty":
        return np.zeros(rows, dtype=bool)
    raise ValueError(case.mask)


def reference_scores(case: Case):
    """(float32 [MAX_QUERIES][rows], float64 the same): the reference's scores of every row under every query of the corpus, once per corpus."""
    key = ("scores", case.corpus)
    if key not in _cache:
        _, held, qs = corpus_arrays(case.corpus)
        with np.errstate(invalid="ignore"):
            s32 = np.stack([vo.scores_full(held, q).astype(np.float32) for q in qs])
            s64 = np.stack([vo.scores_f64(held, q) for q in qs])
        _cache[key] = (s32, s64)
    return _cache[key]


def best_per_message(case: Case, qi: int):
    """top_messages_cases.best_per_message over this table's masks and queries: (float32 reference best score per message ordinal, NaN
    where the message has no allowed row with a score; the same in float64)."""
    rm = message_map(case.corpus.rows, case.map)
    mask = case_mask(case)
    rows = np.arange(case.corpus.rows) if mask is None else np.flatnonzero(mask)
    rows = rows[rm[rows] >= 0]
    n = n_messages(case)
    best32 = np.full(n, np.nan, dtype=np.float32)
    best64 = np.full(n, np.nan, dtype=np.float64)
    s32, s64 = reference_scores(case)
    np.fmax.at(best32, rm[rows], s32[qi][rows])  # (fmax: a NaN row does not hide its message's other rows)
    np.fmax.at(best64, rm[rows], s64[qi][rows])
    return best32, best64


def expected(case: Case, qi: int):
    """The reference's answer: (messages, float32 scores) by (best descending, ordinal ascending), passing the threshold, cut at K."""
    best32, _ = best_per_message(case, qi)
    thr = vo.f32_threshold(threshold_of(case, qi))
    with np.errstate(invalid="ignore"):
        ok = np.flatnonzero(~np.isnan(best32) & (best32 >= thr))
    order = ok[np.lexsort((ok, -best32[ok].astype(np.float64)))][: case_k(case)]
    return order, best32[order]


def best_of_arrays(held: np.ndarray, q: np.ndarray, rm: np.ndarray, mask=None):
    """`best_per_message` for any corpus (float32 rows as the device holds them), query, map and bool mask: what the row-edit tests judge
    a fresh model with."""
    rm = np.asarray(rm, dtype=np.int64)
    rows = np.arange(len(held)) if mask is None else np.flatnonzero(mask)
    rows = rows[rm[rows] >= 0]
    n = int(rm.max()) + 1
    best32 = np.full(n, np.nan, dtype=np.float32)
    best64 = np.full(n, np.nan, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        np.fmax.at(best32, rm[rows], vo.scores_full(held[rows], q).astype(np.float32))
        np.fmax.at(best64, rm[rows], vo.scores_f64(held[rows], q))
    return best32, best64


def judge_lists(best32, best64, dim: int, k: int, threshold: float, got_items, got_scores, name: str = ""):
    """top_messages_cases.judge_b's rules over a best-score vector: scores within SCORE_TOL of the reference's best score of that message,
    non-increasing with ties by ascending ordinal, the ordinals the reference's except among near-ties decided by the float64 referee,
    and the count the reference's wherever no message sits at the threshold.  Returns the report."""
    def referee(positions):
        return best64[np.asarray(positions, dtype=np.int64)]

    referee.dim = dim
    thr = vo.f32_threshold(threshold)
    got_items, got_scores = [int(i) for i in got_items], [float(s) for s in got_scores]
    for a in range(len(got_items) - 1):
        assert got_scores[a] > got_scores[a + 1] or (got_scores[a] == got_scores[a + 1] and got_items[a] < got_items[a + 1]), (
            f"{name}: ranks {a}, {a + 1} out of order: {got_items[a:a + 2]} {got_scores[a:a + 2]}")
    rep = vo.check_topk_parity(best32, got_items, got_scores, k, float(thr), referee=referee)
    if not rep.threshold_ambiguous:  # no message sits at the threshold: the count is the reference's exactly
        with np.errstate(invalid="ignore"):
            want = min(k, int((~np.isnan(best32) & (best32 >= thr)).sum()))
        assert len(got_items) == want, f"{name}: {len(got_items)} messages, the reference has {want}"
    return rep


def judge(case: Case, qi: int, got_items, got_scores):
    """`judge_lists` for query qi of a case of the table."""
    best32, best64 = best_per_message(case, qi)
    return judge_lists(best32, best64, case.corpus.dim, case_k(case), threshold_of(case, qi), got_items, got_scores, f"{case.name} q{qi}")


def expected_kernel(case: Case) -> int:
    """What "last_skinny_kernel" reports for the case: 10000 x variant (0: the ring) + 100 x bytes per K step + queries per tile of the
    LAST group's tile launch."""
    row_bytes = case.corpus.dim * (2 if case.corpus.dtype == "float16" else 4)
    step = 128 if row_bytes % 128 == 0 else 64
    per = group_size(case)
    last = case.nq - (case.nq - 1) // per * per
    return step * 100 + (64 if last > 32 else 32)


def group_size(case: Case) -> int:
    """Queries per tile launch: 64, cut by "topk_scores_bytes" over [queries][n_messages] (at least one)."""
    if not case.scores_bytes:
        return min(64, case.nq)
    return max(1, min(64, case.nq, case.scores_bytes // (4 * n_messages(case))))
