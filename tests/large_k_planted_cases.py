"""TEST INFRASTRUCTURE -- the branch table of the large-k selection and the sorted route (csrc/tavb_topk.hip: find_from_top,
first_bits_at_least, resolve, topk_refine_kernel, topk_compact_kernel, topk_finish_kernel, sorted_count_kernel / sorted_compact_kernel,
message_hist_kernel, and the ScoreSink / MessageMaxSink epilogues of csrc/tavb_scan.hip), shared by tests/test_gpu_large_k_planted.py (the
device) and tests/test_large_k_planted_host.py (its CPU twin).  No torch, no GPU.

Planted scores.  A row [c, 0, 0, ...] against the query e_0 has the dot product c exactly on every tier (one fmaf(c, 1, 0), products
with zero, and a wave sum of zeros), so its score is float32((c + 1) * 0.5) with the clip and the NaN rule of cosine_to_score: the table
chooses the score BITS of every row, numpy gives the expected answer bit for bit, and the oracle agrees exactly.  Every float32 score in
[0.5, 1] can be planted (c = 2 s - 1 is exact there).  In a batch column i carries query i's distribution and query i is e_i (a ninth
query reuses column 0 under another threshold); a row with a NaN anywhere is NaN for every query.  fp16 corpora use cosines that fp16
holds, m / 2048: few distinct scores, many ties.

The host model is a float32 copy of the bucket map (topk_bucket in tavb_device.h, bucket_maps in tavb_lookup_topk.hip) and an integer copy
of first_bits_at_least, topk_refine_rounds and resolve; `branches(case)` is derived from it and from the launch shapes:

  sel_blocks    shape_score_pass / plan_top_messages: min(max(1, ceil(n_pos / 2048)), max(1, 2048 / queries of the group)) workgroups of
                256 threads for topk_refine_kernel, topk_compact_kernel and message_hist_kernel: ONE workgroup up to 2048 positions, so a
                grid stride is 256 positions (tail cases 255 / 256 / 257) and two workgroups begin at 2049
  sorted_blocks b = ceil(n_pos / 2048), chunk = ceil(n_pos / b) rounded up to 256, blocks = ceil(n_pos / chunk): one block up to 2048
                positions, chunk 1280 and two blocks at 2049 .. 2560, chunk 1536 and two blocks at 2561, chunk 1536 and three at 4097

What tests/top_messages_cases.py already covers of tavb_search_top_messages (so this table does not): random corpora of 1 .. 4099 rows at
widths 6 / 8 / 384 / 1536, six row -> message maps (with -1 holes and sparse ordinals), 1 / 2 / 8 / 9 queries, K in {1, 10, 256, 257,
n, n + 5}, thresholds 0 / the 0.9 quantile / 1.5 / per query, five allowed sets, and ONE tie case (600 identical rows, K = 100, a
boundary list of 64).  It has no message whose best row scores exactly 0.0, never sets topk_buckets, has no map value >= n_messages, no K
at the number of passing messages +- 1 chosen on purpose, and no tie at rank K between two runs: those are the message cases here."""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

ONE_BITS = 0x3F800000  # 1.0f: the largest score
REFINE_BUCKETS = 4096  # kTopkRefineBuckets
MAX_STREAM_QUERIES = 8  # queries of one score pass
MAX_LARGE_K = 16384
DEFAULT_BUCKETS, DEFAULT_CAP = 1024, 16384  # "topk_buckets", "topk_boundary_keys"
MAX_CORPUS_ELEMENTS = 3000 * 1536  # the committed size cap of a case's corpus (the tier-1 cases; every other corpus is <= 130 000 x 8)
F32 = np.float32
NAN = float("nan")


# ---------------------------------------------------------------------------------------------------------------- planted scores
def score_of_cosine(c) -> np.ndarray:
    """cosine_to_score (tavb_device.h) in float32: one rounded add, an exact halving, negative and -0 -> +0, above 1 -> 1, NaN stays."""
    c = np.asarray(c, dtype=F32)
    with np.errstate(invalid="ignore"):
        s = (c + F32(1.0)) * F32(0.5)
        s = np.where(s > 0, s, np.where(np.isnan(s), s, F32(0.0)))
        s = np.where(s > 1, F32(1.0), s)
    return s.astype(F32)


def cosine_of_bits(bits) -> np.ndarray:
    """The cosine whose score has exactly these float32 bits (scores in [0.5, 1])."""
    s = np.asarray(bits, dtype=np.uint32).view(F32)
    assert np.all((s >= 0.5) & (s <= 1.0))
    c = (s * F32(2.0) - F32(1.0)).astype(F32)
    assert np.array_equal(score_of_cosine(c).view(np.uint32), np.asarray(bits, dtype=np.uint32))
    return c


C_ONE, C_ZERO, C_HIGH, C_LOW, C_NAN, C_HALF = F32(1.0), F32(-1.0), F32(1.5), F32(-3.0), F32(NAN), F32(0.0)  # the special row kinds


def planted_corpus(cosines, dim: int, dtype: str, axis: int = 0) -> np.ndarray:
    """float32 [rows, dim]: the cosine(s) of each row on `axis` (a [rows, n] array: on axis .. axis + n - 1), zeros elsewhere.  fp16
    corpora must survive the device's conversion unchanged."""
    c = np.asarray(cosines, dtype=F32)
    c = c[:, None] if c.ndim == 1 else c
    v = np.zeros((c.shape[0], dim), dtype=F32)
    v[:, axis : axis + c.shape[1]] = c
    if dtype == "fp16":
        with np.errstate(invalid="ignore"):
            back = v.astype(np.float16).astype(F32)
        assert np.array_equal(back.view(np.uint32), v.view(np.uint32)), "an fp16 corpus must hold cosines fp16 represents"
    return v


# ---------------------------------------------------------------------------------------------------------------- the host model
def bucket_params(thr, nb: int):
    """bucket_maps (tavb_lookup_topk.hip): lo = the threshold brought into [0, 1] (NaN: 0), scale = nb / (1 - lo), 0 at lo = 1."""
    ms = F32(thr)
    lo = ms if ms > 0 else F32(0.0)
    if lo > 1:
        lo = F32(1.0)
    scale = F32(nb) / (F32(1.0) - lo) if lo < 1 else F32(0.0)
    return F32(lo), F32(scale)


def bucket_map(s, lo, scale, nb: int) -> np.ndarray:
    """topk_bucket (tavb_device.h): min(nb - 1, floor((s - lo) * scale)), 0 where the product is not positive -- two rounded float32 operations."""
    s = np.asarray(s, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = ((s - F32(lo)).astype(F32) * F32(scale)).astype(F32)
        inside = (t > 0) & (t < F32(nb - 1))
        low = np.where(inside, t, F32(0.0)).astype(np.int64)
        return np.where(t > 0, np.where(inside, low, nb - 1), 0).astype(np.int64)


def first_bits_at_least(target: int, lo, scale, nb: int) -> int:
    """The smallest score bits in [0, 1.0f] whose bucket is >= target; ONE_BITS + 1 when there is none (the device's bisection)."""
    a, b = 0, ONE_BITS + 1
    while a < b:
        m = a + (b - a) // 2
        if int(bucket_map(np.array([m], dtype=np.uint32).view(F32), lo, scale, nb)[0]) >= target:
            b = m
        else:
            a = m + 1
    return a


@functools.lru_cache(maxsize=None)
def bucket_bits(j: int, thr: float, nb: int) -> tuple[int, int]:
    """(first, last) score bits of bucket j under threshold thr and nb buckets; first > last: the bucket holds no score."""
    lo, scale = bucket_params(thr, nb)
    return first_bits_at_least(j, lo, scale, nb), first_bits_at_least(j + 1, lo, scale, nb) - 1


def topk_refine_rounds(n_pos: int, cap: int) -> int:
    if n_pos <= cap:
        return 0
    w, r = 1 << 62, 0
    while w > cap:
        w = w // REFINE_BUCKETS + 1
        r += 1
    return r


def find_from_top(h: np.ndarray, need: int):
    """(bucket, keys above it, keys in it) where the count from the top first reaches need (1 <= need <= h.sum())."""
    c = np.cumsum(h[::-1])
    i = int(np.searchsorted(c, need))
    b = len(h) - 1 - i
    return b, int(c[i] - h[b]), int(h[b])


def sel_blocks(n_pos: int, per: int) -> int:
    return min(max(1, (n_pos + 2047) // 2048), max(1, 2048 // per))


def sorted_blocks(n_pos: int) -> tuple[int, int]:
    b = min(max((n_pos + 2047) // 2048, 1), 1024)
    c = (n_pos + b - 1) // b
    c = (c + 255) // 256 * 256
    return (n_pos + c - 1) // c, c


@dataclass(frozen=True)
class Model:
    empty: bool
    total: int = 0
    need: int = 0
    above: int = 0  # sure keys after the last round
    inb: int = 0  # keys in the boundary range after the last round
    inb0: int = 0  # keys in the boundary bucket before any round
    above0: int = 0
    rounds: int = 0
    bucket: int = -1
    lane: int = -1  # the lane of find_from_top that owns the bucket
    lane_first: bool = False  # the bucket is the first of that lane's walk (the top of its range)
    lane_last: bool = False
    last_subrange: bool = False  # a round chose the last sub-range of a range its step does not divide
    ka: int = 1
    kb: int = 0
    ka0: int = 1  # the lower end of the boundary bucket's key range, before any round


def row_keys(scores: np.ndarray, pos: np.ndarray) -> np.ndarray:
    return (scores[pos].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - pos.astype(np.uint64))


def passing(scores: np.ndarray, thr) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(scores >= F32(thr))  # NaN (score or threshold) never passes


def run_model(scores: np.ndarray, thr, k: int, nb: int, cap: int, rounds_max: int) -> Model:
    """resolve (tavb_topk.hip) over the positions' scores (float32, NaN: no score) for need = min(k, survivors), in integers after the bucket map."""
    pos = passing(scores, thr)
    total = len(pos)
    if total == 0:
        return Model(empty=True)
    keys = row_keys(scores, pos)
    lo, scale = bucket_params(thr, nb)
    hist = np.bincount(bucket_map(scores[pos], lo, scale, nb), minlength=nb)
    need = min(k, total)
    j, above, inb = find_from_top(hist, need)
    per = nb // 64
    lane = (nb - 1 - j) // per
    ka = first_bits_at_least(j, lo, scale, nb) << 32
    kb = ((first_bits_at_least(j + 1, lo, scale, nb) - 1) << 32) | 0xFFFFFFFF
    above0, inb0, ka0, rounds, last = above, inb, ka, 0, False
    while rounds < rounds_max and inb > cap:
        w = kb - ka + 1
        step = w // REFINE_BUCKETS + (w % REFINE_BUCKETS != 0)
        sel = keys[(keys >= np.uint64(ka)) & (keys <= np.uint64(kb))]
        rh = np.bincount(((sel - np.uint64(ka)) // np.uint64(step)).astype(np.int64), minlength=REFINE_BUCKETS)
        jj, ab, inn = find_from_top(rh, need - above)
        last = last or (w % step != 0 and jj == (w - 1) // step)
        ka = ka + jj * step
        kb = min(ka + step - 1, kb)
        above, inb, rounds = above + ab, inn, rounds + 1
    return Model(False, total, need, above, inb, inb0, above0, rounds, j, lane, j == nb - lane * per - 1, j == nb - (lane + 1) * per, last, ka, kb, ka0)


# ---------------------------------------------------------------------------------------------------------------- corpora and cases
@dataclass(frozen=True)
class Planted:
    cos: np.ndarray  # float32 [rows, columns]: column i is query i's distribution
    dim: int
    dtype: str  # "fp32" / "fp16"
    row_to_msg: np.ndarray | None = None  # message cases: int64 [rows]
    n_messages: int = 0  # (may be smaller than the map's largest value + 1: the values beyond are skipped)
    row_list: np.ndarray | None = None  # message cases over a row list: ascending rows


@dataclass(frozen=True)
class Case:
    name: str
    call: str  # "topk" (search_topk), "sorted" (search_sorted), "messages" (search_top_messages)
    corpus: str  # a key of CORPORA
    k: int
    thr: tuple  # one threshold per query
    buckets: int = DEFAULT_BUCKETS
    cap: int = DEFAULT_CAP
    tier: int = 2  # "last_tier" after the call
    want: tuple = ()  # the branches the case is in the table for (asserted to be among branches(case))
    family: str = ""  # the builder below that made the case: the GPU suite has one test id per family and runs the family's cases in it

    @property
    def nq(self) -> int:
        return len(self.thr)


CORPORA: dict = {}  # name -> builder of a Planted
CASES: list[Case] = []


@functools.lru_cache(maxsize=None)
def corpus_of(name: str) -> Planted:
    return CORPORA[name]()


def vectors(case: Case) -> np.ndarray:
    p = corpus_of(case.corpus)
    return planted_corpus(p.cos, p.dim, p.dtype)


def queries(case: Case) -> np.ndarray:
    p = corpus_of(case.corpus)
    q = np.zeros((case.nq, p.dim), dtype=F32)
    q[np.arange(case.nq), np.arange(case.nq) % p.cos.shape[1]] = 1.0
    return q


def row_scores(case: Case, qi: int) -> np.ndarray:
    """float32 [rows]: the planted formula.  NaN anywhere in a row makes the row NaN for every query (NaN * 0)."""
    p = corpus_of(case.corpus)
    s = score_of_cosine(p.cos[:, qi % p.cos.shape[1]])
    return np.where(np.isnan(p.cos).any(axis=1), F32(NAN), s).astype(F32)


def position_scores(case: Case, qi: int) -> np.ndarray:
    """float32 per position of the selection, NaN: none.  Rows; for a message case message ordinals with the best score of the message's
    passing rows (inside the row list, map values outside [0, n_messages) skipped)."""
    s = row_scores(case, qi)
    if case.call != "messages":
        return s
    p = corpus_of(case.corpus)
    rows = np.arange(len(s)) if p.row_list is None else p.row_list
    rows = rows[(p.row_to_msg[rows] >= 0) & (p.row_to_msg[rows] < p.n_messages)]
    rows = rows[np.isin(rows, passing(s, case.thr[qi]))]
    best = np.full(p.n_messages, NAN, dtype=F32)
    np.fmax.at(best, p.row_to_msg[rows], s[rows])
    return best


def effective_k(case: Case, n_pos: int) -> int:
    return n_pos if case.call == "sorted" and (case.k == 0 or case.k > n_pos) else case.k


def rounds_enqueued(case: Case, n_pos: int) -> int:
    if case.call == "sorted" and effective_k(case, n_pos) >= n_pos:
        return 0  # every survivor: nothing to refine
    return topk_refine_rounds(n_pos, case.cap)


def expected(case: Case, qi: int):
    """(ordinals int64 [m], score bits uint32 [m]): s >= float32(thr), by score descending then ordinal ascending, the first k (all at k = 0)."""
    order, bits = ranked(case, qi)
    k = effective_k(case, len(position_scores(case, qi)))
    return order[:k], bits[:k]


def ranked(case: Case, qi: int):
    """every survivor in the library's order (the keys are unique: descending by key is score descending, then ordinal ascending)"""
    s = position_scores(case, qi)
    pos = passing(s, case.thr[qi])
    order = pos[np.argsort(row_keys(s, pos))[::-1]]
    return order.astype(np.int64), s[order].view(np.uint32)


def model(case: Case, qi: int) -> Model:
    s = position_scores(case, qi)
    return run_model(s, case.thr[qi], effective_k(case, len(s)), case.buckets, case.cap, rounds_enqueued(case, len(s)))


def expected_rounds(case: Case) -> int:
    """"last_topk_refine" after the call: the most rounds of any query of the batch (note_rounds / SortedRun::max_rounds run over every pass)."""
    return max(model(case, q).rounds for q in range(case.nq))


def passes(case: Case) -> list[range]:
    p = corpus_of(case.corpus)
    epl = 8 if p.dtype == "fp16" else 4
    nb = 0 if case.call == "messages" else case.buckets
    if p.dim % epl:
        per = 8 if 8 * nb * 4 <= 150 * 1024 else 4
    else:
        per = MAX_STREAM_QUERIES
        while per > 1 and ((per * p.dim * 4 + 15) & ~15) + per * nb * 4 > 150 * 1024:
            per //= 2
    per = min(per, case.nq)
    return [range(q0, min(q0 + per, case.nq)) for q0 in range(0, case.nq, per)]


def branches(case: Case) -> set[str]:
    out = {f"tier-{case.tier}", f"nq-{case.nq}", f"call-{case.call}", f"buckets-{case.buckets}"}
    n_pos = len(position_scores(case, 0))
    models = [model(case, q) for q in range(case.nq)]
    ps = passes(case)
    if len(ps) > 1:
        out.add("two-passes")
    if n_pos in (63, 64, 65):
        out.add("tail-64")
    if n_pos in (255, 256, 257):
        out.add("tail-256")
    if n_pos == 1:
        out.add("tail-1")
    if n_pos == 256 * sel_blocks(n_pos, len(ps[0])) + 1:
        out.add("stride+1")
    if n_pos == 256 * sel_blocks(n_pos, len(ps[0])) - 1:
        out.add("stride-1")
    if n_pos in (2048, 2049):
        out.add(f"sel-blocks-{sel_blocks(n_pos, len(ps[0]))}")
    for r in ps:
        ms = [models[q] for q in r]
        if any(ms[i].empty and not ms[i - 1].empty and not ms[i + 1].empty for i in range(1, len(ms) - 1)):
            out.add("empty-between")
        rs = {m.rounds for m in ms if not m.empty}
        if 0 in rs and 1 in rs and any(x >= 3 for x in rs):
            out.add("mixed-rounds")
    if len({F32(t).tobytes() for t in case.thr}) > 1:
        out.add("mixed-thresholds")
    for q, m in enumerate(models):
        thr = F32(case.thr[q])
        s = position_scores(case, q)
        k = effective_k(case, n_pos)
        if np.isnan(thr):
            out.add("thr-nan")
        elif thr < 0:
            out.add("thr-neg")
        elif thr == 0:
            out.add("thr-0")
        elif thr > 1:
            out.add("thr-above-1")
        if m.empty:
            out.add("empty")
            continue
        if thr >= 1:
            out.add("scale-0")
        live = s[passing(s, thr)].view(np.uint32)
        dead = s[~np.isnan(s)].view(np.uint32)
        if not np.isnan(thr) and 0 < thr < 1:
            tb = int(thr.view(np.uint32))
            if np.any(live == tb + 1) and not np.any(live == tb):
                out.add("thr-ulp-below")  # the threshold one ulp below a planted score: the row passes
            if np.any(dead == tb - 1) and not np.any(live == tb):
                out.add("thr-ulp-above")  # ... one ulp above: it does not
        out.add("fits" if m.rounds == 0 else f"refine-{m.rounds}")
        if m.need == m.total:
            out.add("need-total")
        if m.need == m.total - 1:
            out.add("need-total-1")
        if m.need == 1:
            out.add("need-1")
        if m.need == k:
            out.add("need-k")
        if m.above0 == m.need - 1 and m.need > 1:
            out.add("sure-exact")  # the sure keys make up all of need but the one key the boundary bucket must give
        if m.above0 == 0:
            out.add("above-0")
        if m.above0 + m.inb0 == m.need < m.total:
            out.add("need-at-bucket-edge")  # the rank-need key is the lowest of its bucket: `>=` in find_from_top, not `>`
        if m.bucket == case.buckets - 1:
            out.add("bucket-top")
        if m.bucket == 0:
            out.add("bucket-0")
        if m.ka0 == 0:
            out.add("ka-0")
        if 0 < m.lane < 63 and m.lane_first:
            out.add("lane-first")
        if 0 < m.lane < 63 and m.lane_last:
            out.add("lane-last")
        for d, tag in ((-1, "inb-cap-1"), (0, "inb-cap"), (1, "inb-cap+1")):
            if m.inb0 == case.cap + d:
                out.add(tag)
        if m.last_subrange:
            out.add("last-subrange")
        out.add("k>cap" if k > case.cap else "k<cap" if k < case.cap else "k=cap")
        o, b = expected(case, q)
        if m.need < m.total and ranked(case, q)[1][m.need] == b[-1]:
            out.add("tie-at-k")
        if case.call == "sorted":
            blocks, chunk = sorted_blocks(n_pos)
            out.add(f"chunk-{blocks}")
            out.add("sorted-k0" if case.k == 0 else "sorted-k>max" if case.k == MAX_LARGE_K + 1 else "sorted-k=n" if case.k == n_pos
                    else "sorted-k=n+1" if case.k == n_pos + 1 else "sorted-k<n")
            if n_pos > MAX_LARGE_K + 1 and m.rounds >= 1:
                out.add("sorted-refine")
            if "tie-at-k" in out and blocks > 1:
                run = np.flatnonzero(s.view(np.uint32) == b[-1])
                if run.min() < chunk <= run.max() and np.all(np.diff(run) == 1):
                    out.add("chunk-tie-straddle")
        if case.call == "messages":
            p = corpus_of(case.corpus)
            m_pass = m.total
            if np.any(b == 0):
                out.add("msg-zero-best")
            if np.any(p.row_to_msg == -1):
                out.add("msg-skip-neg")
            if np.any(p.row_to_msg >= p.n_messages):
                out.add("msg-skip-high")
            for d, tag in ((-1, "msg-k-1"), (0, "msg-k"), (1, "msg-k+1")):
                if case.k == m_pass + d:
                    out.add(tag)
            if p.row_list is not None:
                out.add("msg-row-list")
            if "tie-at-k" in out and case.cap == 64 and m.rounds >= 1:
                out.add("msg-tie-cap64")
    return out


# every name below must be hit by a case (tests/test_large_k_planted_host.py)
REQUIRED = frozenset(
    ["empty", "fits", "refine-1", "refine-2", "refine-3", "refine-4", "refine-5", "need-total", "need-total-1", "need-1", "need-k", "sure-exact", "above-0", "need-at-bucket-edge",
     "bucket-top", "bucket-0", "ka-0", "lane-first", "lane-last", "inb-cap-1", "inb-cap", "inb-cap+1", "last-subrange", "k>cap", "k<cap",
     "tail-1", "tail-64", "tail-256", "stride+1", "stride-1", "sel-blocks-1", "sel-blocks-2", "chunk-1", "chunk-2", "chunk-3",
     "chunk-tie-straddle", "scale-0", "thr-neg", "thr-0", "thr-above-1", "thr-nan", "thr-ulp-below", "thr-ulp-above", "tie-at-k",
     "tier-1", "tier-2", "tier-3", "nq-1", "nq-3", "nq-8", "nq-9", "two-passes", "empty-between", "mixed-rounds", "mixed-thresholds",
     "buckets-256", "buckets-320", "buckets-1024", "buckets-4096", "sorted-k0", "sorted-k>max", "sorted-k=n", "sorted-k=n+1", "sorted-k<n",
     "sorted-refine", "msg-zero-best", "msg-skip-neg", "msg-skip-high", "msg-k-1", "msg-k", "msg-k+1", "msg-row-list", "msg-tie-cap64",
     "call-topk", "call-sorted", "call-messages"])


_family = ""  # set around every builder at the bottom of the module


def _add(name, call, corpus_name, builder, k, thr, **kw):
    CORPORA.setdefault(corpus_name, builder)
    CASES.append(Case(name, call, corpus_name, k, tuple(thr) if isinstance(thr, (tuple, list)) else (thr,), family=_family, **kw))


def _spread_bits(first: int, last: int, n: int) -> np.ndarray:
    """n distinct score bits inside [first, last], evenly spread, descending"""
    assert last - first + 1 >= n, (first, last, n)
    return np.unique(np.linspace(first, last, n).astype(np.uint64)).astype(np.uint32)[::-1] if n > 1 else np.array([last], dtype=np.uint32)


def _shuffled(cos, seed: int) -> np.ndarray:
    cos = np.asarray(cos, dtype=F32)
    return cos[np.random.default_rng(seed).permutation(len(cos))]


def _single(cos, dim=4, dtype="fp32") -> Planted:
    return Planted(np.asarray(cos, dtype=F32).reshape(-1, 1), dim, dtype)


HALF_BITS = 0x3F000000  # 0.5f
LAST_SUBRANGE_BUCKETS = 320


def _layered(thr: float, nb: int, j: int, above: int, inb: int, below: int, seed: int, extra=()) -> np.ndarray:
    """cosines: `above` rows spread over the buckets above j, `inb` distinct scores inside bucket j, `below` rows under it (down to
    max(thr, 0.5); when j is the lowest bucket that passes: rows that fail the threshold), two NaN rows, and `extra`; shuffled."""
    floor = max(HALF_BITS, int(F32(max(thr, 0.0)).view(np.uint32)))
    first, last = bucket_bits(j, thr, nb)
    first, last = max(first, floor), min(last, ONE_BITS)
    parts = [cosine_of_bits(_spread_bits(first, last, inb))]
    if above:
        parts.append(cosine_of_bits(_spread_bits(last + 1, ONE_BITS, above)))
    if below and first - 1 >= floor + below:
        parts.append(cosine_of_bits(_spread_bits(floor, first - 1, below)))
    elif below:
        parts.append(np.full(below, F32(-0.5)))  # score 0.25: under every threshold used with a lowest bucket
    parts += [np.array([C_NAN, C_NAN]), np.asarray(extra, dtype=F32)]
    return _shuffled(np.concatenate(parts), seed)


def _build_counts():
    # the boundary bucket (700 of 1024, thr 0: about 8 000 float32 values wide) holds cap - 1, cap or cap + 1 distinct scores; the sure keys are
    # need - 1 of them (k = above + 1 ... the bucket gives one key) or none (need <= inb; under cap 64: need = total = inb, nothing else passes)
    ks = (257, 300, 4096, 16384)
    i = 0
    for cap in (64, 1024):
        for d in (-1, 0, 1):
            inb = cap + d
            k = ks[i % 4]
            i += 1
            name = f"counts-cap{cap}-inb{inb}-sure-k{k}"
            _add(name, "topk", name, functools.partial(lambda k, inb, sd: _single(_layered(0.0, 1024, 700, k - 1, inb, 50, sd)), k, inb, 100 + i), k, 0.0,
                 cap=cap, want=("sure-exact", f"inb-cap{'+1' if d > 0 else '-1' if d < 0 else ''}"))
            if cap == 1024:
                k0 = (257, 300, 1000)[d + 1]
                name = f"counts-cap{cap}-inb{inb}-none-above-k{k0}"
                _add(name, "topk", name, functools.partial(lambda inb, sd: _single(_layered(0.0, 1024, 700, 0, inb, 50, sd)), inb, 200 + i), k0, 0.0,
                     cap=cap, want=("above-0", "k<cap"))
            else:
                name = f"counts-cap{cap}-inb{inb}-need-total"  # (the bucket's rows and two NaN rows: nothing else passes)
                _add(name, "topk", name, functools.partial(lambda inb, sd: _single(_layered(0.0, 1024, 700, 0, inb, 0, sd)), inb, 300 + i), 257, 0.0,
                     cap=cap, want=("above-0", "need-total", "k>cap"))
    # both sides of cap for k, at the extremes
    _add("counts-k16384-cap64-inb65", "topk", "counts-k16384-cap64", lambda: _single(_layered(0.0, 1024, 600, 16000, 65, 700, 401)), 16384, 0.0, cap=64,
         want=("k>cap", "need-k"))


def _build_need():
    # 400 distinct scores; the threshold is the m-th best score, so exactly m rows pass: m in {0, 1, k - 1, k, k + 1} at k = 300
    bits = _spread_bits(HALF_BITS + 5, ONE_BITS - 7, 400)

    def corpus():
        return _single(_shuffled(np.concatenate([cosine_of_bits(bits), [C_NAN, C_HALF, C_ZERO]]), 500))

    for m, want in ((0, ("empty",)), (1, ("need-1", "need-total")), (299, ("need-total",)), (300, ("need-total", "need-k")), (301, ("need-total-1",))):
        tb = int(bits[m - 1]) if m else int(bits[0]) + 1
        _add(f"need-survivors{m}-k300", "topk", "need-400", corpus, 300, float(np.uint32(tb).view(F32)), want=want)


def _build_buckets():
    for nb in (256, 320, 1024, 4096):
        per = nb // 64
        lane = 20
        spots = (("top", nb - 1, 0.0), ("lane20-first", nb - lane * per - 1, 0.0), ("lane20-last", nb - (lane + 1) * per, 0.0), ("zero", 0, 0.5))
        for what, j, thr in spots:
            above = 0 if what == "top" else 200
            inb = 400 if what == "top" else 150
            extra = (C_ONE,) * 5 + (C_HIGH,) * 2 if what == "top" else (C_HALF,) * 3 if what == "zero" else ()
            cap = 64 if what in ("top", "zero") else DEFAULT_CAP
            name = f"buckets{nb}-{what}"
            want = {"top": ("bucket-top",), "zero": ("bucket-0", "ka-0"), "lane20-first": ("lane-first",), "lane20-last": ("lane-last",)}[what]
            _add(name, "topk", name, functools.partial(lambda thr, nb, j, above, inb, extra, sd: _single(_layered(thr, nb, j, above, inb, 200, sd, extra)),
                                                        thr, nb, j, above, inb, extra, 600 + nb + j), 300, thr, buckets=nb, cap=cap,
                 want=want + (f"buckets-{nb}",))
    # bucket 0 at threshold 0: 150 rows that score exactly 0.0 (c = -1 and the clipped c = -3) under 200 others, a boundary list of 64 --
    # the range starts at key 0 and every key in it has score bits 0
    _add("buckets1024-zero-score0", "topk", "buckets1024-zero-score0",
         lambda: _single(_shuffled(np.concatenate([cosine_of_bits(_spread_bits(HALF_BITS, ONE_BITS, 200)), np.full(100, C_ZERO), np.full(50, C_LOW), [C_NAN]]), 650)),
         300, 0.0, cap=64, want=("bucket-0", "ka-0", "tie-at-k", "refine-5"))


def _run_corpus(kind: str, run: int, above: int, below: int, thr: float, nb: int, j: int, seed: int) -> Planted:
    first, last = bucket_bits(j, thr, nb)
    mid = (first + last) // 2
    if kind == "identical":
        bits = np.full(run, mid, dtype=np.uint32)
    elif kind == "ulp":
        assert mid + run <= last
        bits = (mid + np.arange(run)).astype(np.uint32)
    elif kind == "ulp4096":
        bits = (first + 4096 * np.arange(run)).astype(np.uint32)  # (leaves the bucket: a few rows per bucket, nothing to refine)
        assert bits.max() < ONE_BITS - 4096 * 8
    else:  # two runs of identical scores, one ulp apart, that meet inside the bucket
        bits = np.concatenate([np.full(run // 2, mid, dtype=np.uint32), np.full(run - run // 2, mid - 1, dtype=np.uint32)])
    top = int(bits.max())
    parts = [cosine_of_bits(bits), cosine_of_bits(_spread_bits(max(top, last) + 1, ONE_BITS, above)), cosine_of_bits(_spread_bits(HALF_BITS, first - 1, below)), [C_NAN]]
    return _single(_shuffled(np.concatenate(parts), seed))


def _build_depth():
    # more than cap rows at each spacing, straddling rank k: the answer depends on position order; the round count is the model's
    for cap, run, above, k in ((64, 300, 200, 300), (1024, 1500, 100, 700)):
        for kind in ("identical", "ulp", "ulp4096", "two-runs"):
            nb, j = (256, 130) if kind == "ulp4096" else (1024, 640)
            name = f"depth-{kind}-cap{cap}"
            kk = above + run // 2 if kind == "two-runs" else k  # (two runs: rank k is the last row of the upper run)
            _add(name, "topk", name, functools.partial(_run_corpus, kind, run, above, 100, 0.0, nb, j, 700 + cap), kk, 0.0, buckets=nb, cap=cap)
            if kind == "identical":
                # need == the sure keys exactly: the count from the top reaches need on the LAST key of a sparse bucket above the run, so
                # the boundary must stop there (no round); a search that walked on would land in the run's bucket and refine it
                _add(name + "-need-at-edge", "topk", name, functools.partial(_run_corpus, kind, run, above, 100, 0.0, nb, j, 700 + cap), above, 0.0, buckets=nb,
                     cap=cap, want=("need-at-bucket-edge", "fits"))
            if kind == "two-runs":
                _add(name + "-k+1", "topk", name, functools.partial(_run_corpus, kind, run, above, 100, 0.0, nb, j, 700 + cap), kk + 1, 0.0, buckets=nb, cap=cap)


def _last_subrange_case():
    """The keys that decide rank k in the last sub-range of a round whose step does not divide the range.  The first two rounds divide
    evenly (the bucket spans nbits << 32 keys, then nbits << 20, then nbits << 8); round three's step is ceil(nbits / 16), so with nbits no
    multiple of 16 its last sub-range is short, and `resolve` must clip kb to the range's end.  A run of identical scores at the i-th score
    value of the bucket is cut by a round-two boundary r positions in (r = ((i + 1) << 32) mod (nbits << 8)); with k a little above r the rank
    falls into the top -- the last -- sub-range of the range under that boundary, which holds more than 64 keys, so a fourth round follows
    over the clipped range.  Without the clip that round counts rows of the run twice."""
    nb, cap, thr = LAST_SUBRANGE_BUCKETS, 64, 0.0  # (1024 buckets at threshold 0 are 16384 values wide each: every step divides)
    for j in range(nb * 5 // 8, nb * 7 // 8):
        first, last = bucket_bits(j, thr, nb)
        nbits = last - first + 1
        w3 = nbits << 8
        step3 = -(-w3 // REFINE_BUCKETS)
        rem = w3 % step3
        if rem <= cap + 8:
            continue
        rs = ((np.arange(1, nbits + 1, dtype=np.uint64) << np.uint64(32)) % np.uint64(w3)).astype(np.int64)
        for i in np.flatnonzero((rs >= 400) & (rs <= 4000)).tolist():
            r = int(rs[i])
            run = r + 1500
            cos = np.concatenate([cosine_of_bits(np.full(run, first + i, dtype=np.uint32)), cosine_of_bits(_spread_bits(HALF_BITS, first - 1, 100)), [C_NAN]])
            k = r + 10
            m = run_model(score_of_cosine(cos), thr, k, nb, cap, topk_refine_rounds(len(cos), cap))
            if m.last_subrange and m.rounds == 4:
                return cos, k
    raise AssertionError("no last-sub-range case found")


def _build_last_subrange():
    @functools.lru_cache(maxsize=None)
    def found():
        return _last_subrange_case()

    _add("last-subrange-cap64", "topk", "last-subrange", lambda: _single(found()[0]), found()[1], 0.0, buckets=LAST_SUBRANGE_BUCKETS, cap=64,
         want=("last-subrange", "refine-4"))


def _build_thresholds():
    bits = _spread_bits(HALF_BITS + 3, ONE_BITS - 3, 600)

    def corpus():
        return _single(_shuffled(np.concatenate([cosine_of_bits(bits), [C_ONE] * 5, [C_HIGH] * 2, [C_NAN, C_ZERO, C_LOW, C_HALF]]), 800))

    for what, thr, want in (("neg", -0.2, ("thr-neg",)), ("zero", 0.0, ("thr-0",)), ("one", 1.0, ("scale-0", "bucket-0")), ("above-one", 1.5, ("thr-above-1", "empty")),
                            ("nan", NAN, ("thr-nan", "empty")),
                            ("ulp-below", float(np.uint32(int(bits[100]) - 1).view(F32)), ("thr-ulp-below",)),
                            ("ulp-above", float(np.uint32(int(bits[100]) + 1).view(F32)), ("thr-ulp-above",))):
        _add(f"thr-{what}", "topk", "thr-600", corpus, 300, thr, cap=64, want=want)
        _add(f"thr-{what}-sorted", "sorted", "thr-600", corpus, 0, thr, want=want)


def _half_run(n: int, seed: int) -> np.ndarray:
    """n cosines: the lower-scoring half distinct, the upper half one identical score (the rank n // 2 + 1 falls inside... the run)"""
    run = (n + 1) // 2
    bits = np.concatenate([np.full(run, HALF_BITS + 0x300000, dtype=np.uint32), _spread_bits(HALF_BITS + 16, HALF_BITS + 0x200000, n - run) if n > run else np.zeros(0, np.uint32)])
    return _shuffled(cosine_of_bits(bits), seed)


def _build_tails():
    # n_pos around a wave and around the one-workgroup grid stride (256 threads: sel_blocks is 1 up to 2048 positions), then where the
    # second workgroup begins; k inside the identical run, a boundary list of 64: wave_append with dead lanes on both lists
    for n in (1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049):
        k = max(1, n // 4)
        _add(f"tail-n{n}-k{k}", "topk", f"tail-n{n}", functools.partial(lambda n: _single(_half_run(n, 900 + n)), n), k, 0.0, cap=64)
        _add(f"tail-n{n}-k300", "topk", f"tail-n{n}", functools.partial(lambda n: _single(_half_run(n, 900 + n)), n), 300, 0.0, cap=64)


def _grid_cosines(n: int, seed: int) -> np.ndarray:
    """n cosines fp16 holds (m / 2048 in [0.5, 1)): about 1000 distinct scores, so ties everywhere; a NaN row and a zero row among them"""
    rng = np.random.default_rng(seed)
    c = (rng.integers(1024, 2048, size=n).astype(F32) / F32(2048.0)).astype(F32)
    c[n // 3] = C_NAN
    c[n // 2] = C_HALF
    return c


def _build_tiers():
    for dtype in ("fp32", "fp16"):
        _add(f"tier1-d1536-{dtype}", "topk", f"tier-d1536-{dtype}", functools.partial(lambda dt: _single(_grid_cosines(3000, 1000), 1536, dt), dtype), 300, 0.0,
             cap=64, tier=1, want=("tier-1",))
        _add(f"tier1-d1536-{dtype}-sorted", "sorted", f"tier-d1536-{dtype}", functools.partial(lambda dt: _single(_grid_cosines(3000, 1000), 1536, dt), dtype), 0, 0.6,
             tier=1, want=("tier-1",))
        _add(f"tier3-d3-{dtype}", "topk", f"tier-d3-{dtype}", functools.partial(lambda dt: _single(_grid_cosines(3000, 1001), 3, dt), dtype), 300, 0.0,
             cap=64, tier=3, want=("tier-3",))
        _add(f"tier3-d3-{dtype}-sorted", "sorted", f"tier-d3-{dtype}", functools.partial(lambda dt: _single(_grid_cosines(3000, 1001), 3, dt), dtype), 2000, 0.0,
             cap=64, tier=3, want=("tier-3",))


def _batch_corpus(ncols: int, dim: int, dtype: str, seed: int) -> Planted:
    """700 rows; the columns cycle through four distributions: distinct scores (no round), 65 scores inside one bucket under the rest (one
    round at a boundary list of 64), one identical run (four rounds; on the fp16 grid too), distinct again (the query that is given
    threshold 1.5 and stays empty)."""
    n = 700
    cols = []
    for i in range(ncols):
        kind = i % 4
        if dtype == "fp16":
            c = _grid_cosines(n, seed + i)
            if kind == 2:
                c[100:500] = F32(1536.0 / 2048.0)
            if kind == 1:  # 65 of the 16 grid scores of one bucket ... ties: the grid cannot hold 65 distinct scores in a bucket
                c[200:265] = F32(1700.0 / 2048.0)
        elif kind in (0, 3):
            c = _shuffled(cosine_of_bits(_spread_bits(HALF_BITS + 9, ONE_BITS - 9, n)), seed + i)
        elif kind == 1:
            c = _layered(0.0, 1024, 700, 280, 65, 353, seed + i)  # 280 + 65 + 353 + 2 NaN = 700
        else:
            c = _shuffled(np.concatenate([cosine_of_bits(np.full(400, bucket_bits(640, 0.0, 1024)[0] + 77, dtype=np.uint32)),
                                          cosine_of_bits(_spread_bits(bucket_bits(660, 0.0, 1024)[0], ONE_BITS, 200)),
                                          cosine_of_bits(_spread_bits(HALF_BITS, bucket_bits(600, 0.0, 1024)[0], 100))]), seed + i)
        cols.append(np.nan_to_num(c, nan=0.0) if i else c)  # (NaN rows are planted through column 0: a NaN makes the row NaN for every query)
    return Planted(np.stack(cols, axis=1).astype(F32), dim, dtype)


def _build_batches():
    # query i: column i % columns; thresholds per query (index 3 of every four is 1.5: empty, between full ones); k = 300, cap = 64
    cyc = (0.0, 0.0, 0.0, 1.5, 0.55, -0.2, 0.0, 1.5, 0.52)
    for nq, dim, dtypes in ((1, 4, ("fp32",)), (3, 4, ("fp32",)), (4, 4, ("fp32",)), (8, 8, ("fp32", "fp16")), (9, 8, ("fp32", "fp16"))):
        for dtype in dtypes:
            ncols = min(nq, dim, 8)
            cname = f"batch-c{ncols}-d{dim}-{dtype}"
            thr = cyc[:nq] if nq != 3 else (0.0, 1.5, 0.0)
            for call, k in (("topk", 300), ("sorted", 300), ("sorted", 0)):
                _add(f"batch-q{nq}-d{dim}-{dtype}-{call}-k{k}", call, cname, functools.partial(_batch_corpus, ncols, dim, dtype, 1100 + nq), k, thr, cap=64)


def _build_sorted():
    def mixed(n, seed):
        run = n // 3
        bits = np.concatenate([np.full(run, HALF_BITS + 0x280000, dtype=np.uint32), _spread_bits(HALF_BITS + 16, ONE_BITS - 16, n - run - 2)])
        return _single(_shuffled(np.concatenate([cosine_of_bits(bits), [C_NAN, C_HALF]]), seed))

    for k in (0, MAX_LARGE_K + 1, 3000, 3001, 1500):
        for thr in (0.0, 0.7):
            _add(f"sorted-n3000-k{k}-thr{thr}", "sorted", "sorted-n3000", functools.partial(mixed, 3000, 1200), k, thr, cap=64)
    # around one block (2048), the two-block chunk of 1280 (2049 .. 2560), chunk 1536 (2561: two blocks; 4097: three)
    for n in (2047, 2048, 2049, 2559, 2560, 2561, 4096, 4097):
        for k in (0, n // 2):
            _add(f"sorted-n{n}-k{k}", "sorted", f"sorted-n{n}", functools.partial(mixed, n, 1300 + n), k, 0.0, cap=64)

    # a run of identical scores in position order across the block boundary (chunk 1280 at 2049 rows) that also crosses rank k
    def straddle():
        n = 2049
        bits = _spread_bits(HALF_BITS + 16, HALF_BITS + 0x100000, n)
        bits[1100:1500] = HALF_BITS + 0x300000  # the run: positions 1100 .. 1499, the best score of the corpus
        return _single(cosine_of_bits(bits))

    for cap in (64, DEFAULT_CAP):
        _add(f"sorted-chunk-tie-straddle-cap{cap}", "sorted", "sorted-straddle", straddle, 250, 0.0, cap=cap, want=("chunk-tie-straddle", "chunk-2"))

    # more than 16 385 rows, k above the device top-k, a boundary bucket (5000 identical rows across rank k) that needs refinement
    def big():
        bits = np.concatenate([np.full(5000, HALF_BITS + 0x280000, dtype=np.uint32), _spread_bits(HALF_BITS + 0x290000, ONE_BITS, 14_000),
                               _spread_bits(HALF_BITS, HALF_BITS + 0x270000, 1000)])
        return _single(_shuffled(cosine_of_bits(bits), 1400))

    _add("sorted-n20000-k17000-refine", "sorted", "sorted-n20000", big, 17_000, 0.0, cap=64, want=("sorted-refine",))


def _build_messages():
    # 900 rows in 300 messages of three (row r: message r // 3); message m's best row scores grade[m]; rows 1 and 2 of a message score less
    def corpus(kind: str) -> Planted:
        n_msg = 300
        best = _spread_bits(HALF_BITS + 64, ONE_BITS - 64, n_msg)  # descending with the message ordinal
        if kind == "tie":  # messages 50 .. 249 share one best score: a tie at rank K decided by the ordinal, 200 > 64 keys in the bucket
            best = best.copy()
            best[50:250] = best[150]
        c = np.repeat(cosine_of_bits(best), 3)
        c[1::3] = C_HALF  # 0.5
        c[2::3] = F32(-0.25)  # 0.375
        rm = np.arange(900, dtype=np.int64) // 3
        n_messages = n_msg
        if kind == "zero":  # messages 290 .. 299: every row scores exactly 0.0 (c = -1 and the clipped c = -3)
            c[870:] = C_ZERO
            c[871::3] = C_LOW
        if kind == "skip":  # rows without a message (-1) and rows whose ordinal is >= n_messages: the best rows of the corpus among them
            rm[0:3] = -1
            rm[3:6] = 400
            rm[30] = -1
            n_messages = 300
        rows = None
        if kind == "list":  # a row list: every row but the best row of each even message below 100
            rows = np.setdiff1d(np.arange(900), np.arange(0, 300, 6)).astype(np.int64)
        return Planted(c.reshape(-1, 1).astype(F32), 4, "fp32", rm, n_messages, rows)

    # a message whose best row scores 0.0: returned at threshold 0 and at a negative threshold, through the `bits + 1` slot encoding
    for thr in (0.0, -0.5):
        _add(f"msg-zero-best-thr{thr}", "messages", "msg-zero", functools.partial(corpus, "zero"), 300, thr, want=("msg-zero-best",))
    _add("msg-zero-best-buckets4096-cap64", "messages", "msg-zero", functools.partial(corpus, "zero"), 295, 0.0, buckets=4096, cap=64, want=("msg-zero-best", "buckets-4096"))
    _add("msg-buckets4096", "messages", "msg-plain", functools.partial(corpus, "plain"), 100, 0.0, buckets=4096, want=("buckets-4096",))
    _add("msg-skip", "messages", "msg-skip", functools.partial(corpus, "skip"), 300, 0.0, want=("msg-skip-neg", "msg-skip-high"))
    # K around the number of messages with a passing row: the threshold passes the best rows of messages 0 .. 119 only
    thr120 = float(_spread_bits(HALF_BITS + 64, ONE_BITS - 64, 300)[119:120].view(F32)[0])
    for k, tag in ((119, "msg-k-1"), (120, "msg-k"), (121, "msg-k+1")):
        _add(f"msg-pass120-k{k}", "messages", "msg-plain", functools.partial(corpus, "plain"), k, thr120, want=(tag,))
        _add(f"msg-pass120-k{k}-list", "messages", "msg-list", functools.partial(corpus, "list"), k - 17, thr120, want=("msg-row-list",))
    for k in (100, 150, 249, 250, 251):
        _add(f"msg-tie-k{k}-cap64", "messages", "msg-tie", functools.partial(corpus, "tie"), k, 0.0, cap=64, want=("msg-tie-cap64",) if k < 250 else ())
    _add("msg-tie-batch", "messages", "msg-tie", functools.partial(corpus, "tie"), 150, (0.0, 1.5, 0.6), cap=64, want=("msg-tie-cap64", "empty-between"))


for _b in (_build_counts, _build_need, _build_buckets, _build_depth, _build_last_subrange, _build_thresholds, _build_tails, _build_tiers, _build_batches,
           _build_sorted, _build_messages):
    _family = _b.__name__[len("_build_"):].replace("_", "-")
    _b()

FAMILIES = tuple(dict.fromkeys(c.family for c in CASES))  # in table order

# the three whole-corpus cases also run through VectorBase.fuzzy_lookup_embedding(s): one that fits, one that refines, one sorted
CLASS_CASES = ("counts-cap64-inb63-sure-k257", "depth-identical-cap64", "sorted-n3000-k0-thr0.7")
