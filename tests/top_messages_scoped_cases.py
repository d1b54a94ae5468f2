"""TEST INFRASTRUCTURE -- the case table of the scoped top-k distinct message lookups (`VectorBase.lookup_top_messages_by_embeddings_scoped`,
tavb_search_top_messages_scoped: one scope PER QUERY), shared by tests/test_gpu_top_messages_scoped.py (the device) and
tests/test_top_messages_scoped_host.py (its CPU twin, which pins the table's own claims).

Semantics under test, per query e_i, threshold t_i, scope s_i and K: `lookup_top_messages_by_embedding(e_i, K, t_i, s_i)` -- of the rows of
s_i whose message is not -1 and whose score is >= t_i, the best score per message, the K best messages by (score descending, ordinal
ascending).  A message whose chunks lie in several queries' scopes gets, for query i, the max over the rows of s_i ONLY.

The corpora, maps, collapse and thresholds are tests/top_messages_cases.py's, the scope families tests/scoped_batch_cases.py's, rebuilt here
over this table's shapes: the smallest at which a piece can go wrong -- 1 row; 31 / 32 / 33 rows around a mask word; 257 past a 256-row
mask chunk; 1000 and 4099 rows for several workgroups; widths 6 (the scalar tier), 8, 72 (fp16 rows that are no multiple of a wave's
1 KiB) and 1536; batches of 1, 2, 8, 9 (a trailing pass of one query) and 17.  `CASES` shuffles the axes against one another with a fixed
seed so that every value of every axis appears, then adds by hand the pairs that each take another path (`HAND`)."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import top_messages_cases as tc
from tests.synth import make_queries
from tests.top_messages_cases import Corpus, collapse, message_map, tenth_threshold  # noqa: F401 -- re-exported to the two test files

CORPORA = (
    Corpus(1, 8, "float32", 9701), Corpus(31, 6, "float16", 9702), Corpus(32, 8, "float16", 9703), Corpus(33, 8, "float32", 9704),
    Corpus(33, 72, "float16", 9705), Corpus(257, 6, "float32", 9706), Corpus(257, 1536, "float32", 9707), Corpus(1000, 72, "float16", 9708),
    Corpus(1000, 8, "float32", 9709), Corpus(4099, 1536, "float16", 9710), Corpus(4099, 8, "float32", 9711),
)
ROWS = (1, 31, 32, 33, 257, 1000, 4099)
WIDTHS = (6, 8, 72, 1536)
MAPS = tc.MAPS
BATCHES = (1, 2, 8, 9, 17)
KS = (1, 10, 257, "n", "n+5")
THRESHOLDS = ("zero", "tenth", "above", "per_query")
FAMILIES = ("identical", "disjoint", "nested", "random1%", "random50%", "one_empty", "first_row", "last_row", "all_rows", "all_empty")
# how the scopes reach the class: the bool arrays themselves, `row_mask` handles, `message_mask` / `range_mask(of="messages")` handles
# (the "by_message" family only), or handles one of which has no packed mask on the device (the class must loop)
FORMS = ("raw", "handles", "message_handles", "host_only")
MAX_QUERIES = 17
ORDINAL_BASE = 1_000_003
MAX_LARGE_K = 16384


@dataclass(frozen=True)
class Case:
    corpus: Corpus
    map: str
    nq: int
    k: object  # an int, "n" (= n_messages) or "n+5"
    thresholds: str
    family: str
    form: str = "handles"
    note: str = ""  # hand-added cases: what they are there for

    @property
    def name(self) -> str:
        return f"{self.corpus.name}-{self.map}-q{self.nq}-k{self.k}-{self.thresholds}-{self.family}-{self.form}{'-' + self.note if self.note else ''}"

    @property
    def seed(self) -> int:
        return 9700 + 7 * (FAMILIES + ("cycle5", "by_message")).index(self.family) + 131 * self.corpus.rows + 17 * self.nq


def _table() -> list[Case]:
    # six cases per corpus; every other axis is its values repeated to that length and shuffled (fixed seed), as in the two parent tables
    n = 6 * len(CORPORA)
    rng = np.random.default_rng(9700)

    def axis(values):
        return [values[j] for j in rng.permutation(np.arange(n) % len(values))]

    maps, nqs, ks, thrs, fams, forms = axis(MAPS), axis(BATCHES), axis(KS), axis(THRESHOLDS), axis(FAMILIES), axis(("raw", "handles"))
    return [Case(CORPORA[i % len(CORPORA)], maps[i], nqs[i], ks[i], thrs[i], fams[i], forms[i]) for i in range(n)]


_BIG16, _SMALL32, _MID16 = CORPORA[9], CORPORA[3], CORPORA[7]
# the cases added by hand, by the number the issue gives them
HAND = {
    # 1. every message has chunks in several queries' scopes: a wrong membership bit shows up as a too-high score
    "1a": Case(CORPORA[8], "interleaved", 8, 10, "zero", "disjoint", "handles", "hand1"),
    "1b": Case(_BIG16, "interleaved", 9, "n", "zero", "disjoint", "handles", "hand1"),
    # 2. all rows are message 0: each query's single score is its own scope's max
    "2": Case(_MID16, "one", 8, 10, "zero", "disjoint", "handles", "hand2"),
    # 3. nine queries at 4099 x 1536 fp16 with "topk_scores_bytes" at its floor: every pass splits into sub-groups with bit0 > 0
    "3": Case(_BIG16, "chunks3", 9, 10, "per_query", "nested", "handles", "hand3-floor"),
    # 4. 129 queries: more than 16 passes, so a second wave runs
    "4": Case(_SMALL32, "chunks3", 129, 10, "per_query", "cycle5", "handles", "hand4-waves"),
    # 5. an adopted device corpus whose row ordinals start at ORDINAL_BASE: message ordinals must not carry it
    "5": Case(_MID16, "chunks3", 9, 10, "per_query", "nested", "handles", "hand5-adopted"),
    # 6. the forms of a scope: raw arrays and row_mask handles (also in the shuffle), message_mask / range_mask handles, a host-only handle
    "6a": Case(_MID16, "holes", 8, 25, "tenth", "random50%", "raw", "hand6"),
    "6b": Case(_MID16, "holes", 8, 25, "tenth", "random50%", "handles", "hand6"),
    "6c": Case(_MID16, "interleaved", 9, 25, "zero", "by_message", "message_handles", "hand6"),
    "6d": Case(_MID16, "chunks3", 3, 25, "zero", "random50%", "host_only", "hand6"),
}
FLOOR_BYTES = 4096  # the floor of the engine option "topk_scores_bytes"

CASES = _table() + list(HAND.values())
TABLE_CASES = [c for c in CASES if c.note not in ("hand5-adopted",)]  # what runs on the corpus' shared index
B_CASES = [next(c for c in CASES if c.corpus == corpus and c.family not in ("identical", "all_empty") and 1 < c.nq <= tc.MAX_QUERIES and c.thresholds != "above"
                and c.form in ("raw", "handles") and c.note == "") for corpus in CORPORA if corpus.rows > 1]

_queries: dict = {}


def corpus_arrays(c: Corpus):
    """(rows as handed to the index, rows as the device holds them, MAX_QUERIES queries): tests/top_messages_cases.py's rows (one NaN row
    and one all-zero row from 63 rows on) under this table's longer batch."""
    v, held, _ = tc.corpus_arrays(c)
    if c not in _queries:
        _queries[c] = make_queries(MAX_QUERIES, c.dim, c.seed + 50)
    return v, held, _queries[c]


def case_queries(case: Case) -> np.ndarray:
    """float32 [nq, dim]: the corpus' queries, repeating from MAX_QUERIES on."""
    qs = corpus_arrays(case.corpus)[2]
    return np.ascontiguousarray(qs[np.arange(case.nq) % MAX_QUERIES])


def n_messages(case: Case) -> int:
    return int(message_map(case.corpus.rows, case.map).max()) + 1


def case_k(case: Case) -> int:
    n = n_messages(case)
    return n if case.k == "n" else n + 5 if case.k == "n+5" else int(case.k)


def case_thresholds(case: Case):
    """One float, or a list with one threshold per query."""
    if case.thresholds == "zero":
        return 0.0
    if case.thresholds == "above":
        return 1.5
    t = tenth_threshold(case.corpus)
    if case.thresholds == "tenth":
        return t
    return [(0.0, t, 1.5, 0.5)[i % 4] for i in range(case.nq)]


def threshold_of(case: Case, qi: int) -> float:
    t = case_thresholds(case)
    return t[qi] if isinstance(t, list) else t


def scope_specs(case: Case) -> list[tuple]:
    """The "by_message" family as the caller states it, one entry per query: ("messages", ordinals) for `message_mask`, or ("ranges",
    collections) for `range_mask(..., of="messages")`.  Two queries share one spec OBJECT."""
    assert case.family == "by_message"
    n, nq = n_messages(case), case.nq
    specs: list[tuple] = []
    for q in range(nq):
        if q % 2 == 0:
            specs.append(("messages", np.concatenate([np.arange(q, n, nq + 1, dtype=np.int64), [-1, n + 3]])))
        else:
            lo = (q * n) // (2 * nq)
            specs.append(("ranges", [[(lo, lo + max(1, n // 3))], [(0, n)]]))
    if nq > 2:
        specs[-1] = specs[0]
    return specs


def spec_bools(case: Case, spec: tuple) -> np.ndarray:
    rm = message_map(case.corpus.rows, case.map)
    kind, what = spec
    if kind == "messages":
        return np.isin(rm, what) & (rm >= 0)
    ok = rm >= 0
    for collection in what:
        inside = np.zeros(len(rm), dtype=bool)
        for lo, hi in collection:
            inside |= (rm >= lo) & (rm < hi)
        ok &= inside
    return ok


def case_scopes(case: Case) -> list[np.ndarray]:
    """One bool [rows] array per query; queries that share a scope share the array OBJECT (tests/scoped_batch_cases.py's families, and
    "cycle5": five distinct random masks the queries cycle through; "by_message": the truth of `scope_specs`)."""
    n, nq, fam = case.corpus.rows, case.nq, case.family
    rng = np.random.default_rng(case.seed)
    if fam == "identical":
        return [rng.random(n) < 0.5] * nq
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
    if fam == "all_rows":  # every scope all rows, each its own object
        return [np.ones(n, dtype=bool) for _ in range(nq)]
    if fam == "all_empty":
        return [np.zeros(n, dtype=bool) for _ in range(nq)]
    if fam == "cycle5":
        five = [rng.random(n) < 0.5 for _ in range(5)]
        return [five[q % 5] for q in range(nq)]
    if fam == "by_message":
        made: dict[int, np.ndarray] = {}
        return [made.setdefault(id(s), spec_bools(case, s)) for s in scope_specs(case)]
    raise ValueError(fam)


def expect_native(case: Case) -> bool:
    """Whether the class hands the case to tavb_search_top_messages_scoped: at least two distinct scope objects, something to search,
    1 <= K <= 16384 and every handle with its packed mask on the device."""
    scopes = case_scopes(case)
    return (len({id(s) for s in scopes}) > 1 and any(s.any() for s in scopes) and 1 <= case_k(case) <= MAX_LARGE_K
            and case.form != "host_only")


def judge_b(case: Case, qi: int, got_items, got_scores):
    """`top_messages_cases.judge_b` for query qi over that query's OWN scope: the parent table's judge with this case's scope in the place
    of its allowed set (qi < the parent's nine queries: the first nine of this table's are the same)."""
    assert qi < tc.MAX_QUERIES
    scope = case_scopes(case)[qi]
    proxy = tc.Case(case.corpus, case.map, case.nq, case.k, case.thresholds, "scope")
    saved = tc.case_mask
    tc.case_mask = lambda _case: scope
    try:
        return tc.judge_b(proxy, qi, got_items, got_scores)
    finally:
        tc.case_mask = saved


def passes(nq: int, per: int = 8) -> list[int]:
    """The queries of every pass of the native call."""
    return [min(per, nq - q0) for q0 in range(0, nq, per)]


def sink_best(member: np.ndarray, bit0: int, n_live: int, scores: np.ndarray, passing: np.ndarray, msgs: np.ndarray, n_msgs: int) -> np.ndarray:
    """`ScopedMessageMaxSink` in numpy, for one launch: member uint8 [P] (the membership bytes of the pass' union list), the launch's
    queries = member bits bit0 .. bit0 + n_live - 1, scores float32 [n_live, P] and passing bool [n_live, P] per union position, msgs
    int64 [P] = row_to_msg[row_ids[p]] -> uint32 [n_live, n_msgs]: 1 + the score bits of the best passing member row, 0 = none."""
    best = np.zeros((n_live, n_msgs), dtype=np.uint32)
    for q in range(n_live):
        bit = ((member >> np.uint8(bit0 + q)) & 1).astype(bool)
        take = bit & passing[q] & (msgs >= 0) & (msgs < n_msgs)
        np.maximum.at(best[q], msgs[take], scores[q][take].view(np.uint32) + np.uint32(1))
    return best
