"""TEST INFRASTRUCTURE -- the case table of the scoped message lookups, shared by tests/test_gpu_message_scope.py (the device) and
tests/test_message_scope_host.py (its CPU twin, which pins the table's own claims against numpy).

Mask kernel cases (`MASK_CASES`): a row -> message map, a corpus length and a handful of accept sets each.  `twin_mask_words` restates
`mask_from_messages_kernel` in numpy -- rounds of 64 rows, one vote per lane, two words per ballot -- and is what the device words are
compared with, whole words, tail bits included.

Lookup cases (`LOOKUP_CASES`): three corpora of 3000 rows (64 wide in fp16 and fp32; 72 wide in fp16, a width the 32/64-query tile does
not take), one map of about 1000 messages of 1 to 5 chunks with some rows mapped to -1, and a covering selection of (queries,
max_matches, scope, thresholds) under each forced route.  `expected_route` says which masked route must have run."""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

MASK_ROWS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000, 4097)
MASK_MESSAGES = (1, 31, 33, 700)
MASK_LAYOUTS = ("contiguous", "interleaved")


@dataclass(frozen=True)
class MaskCase:
    rows: int
    n_messages: int
    layout: str
    seed: int

    @property
    def name(self) -> str:
        return f"r{self.rows}-m{self.n_messages}-{self.layout}"


MASK_CASES = [MaskCase(r, m, lay, 9000 + 97 * i + 13 * j + k) for i, r in enumerate(MASK_ROWS) for j, m in enumerate(MASK_MESSAGES)
              for k, lay in enumerate(MASK_LAYOUTS)]


def message_map(n_messages: int, length: int, layout: str, seed: int, holes: float = 0.1) -> np.ndarray:
    """int64 [length]: messages 0 .. n_messages - 1 of 1 to 5 chunks each, laid out contiguously (message after message, from a random first
    row) or interleaved (their chunks scattered over the whole map); what is left over, and a share `holes` of the chunks, is -1."""
    rng = np.random.default_rng(seed)
    chunks = np.repeat(np.arange(n_messages, dtype=np.int64), rng.integers(1, 6, size=n_messages))[:length]
    out = np.full(length, -1, dtype=np.int64)
    if layout == "contiguous":
        start = int(rng.integers(0, length - len(chunks) + 1))
        out[start:start + len(chunks)] = chunks
    elif layout == "interleaved":
        out[np.sort(rng.permutation(length)[: len(chunks)])] = rng.permutation(chunks)
    else:
        raise ValueError(layout)
    out[(out >= 0) & (rng.random(length) < holes)] = -1
    return out


def mask_case_map(case: MaskCase) -> np.ndarray:
    """The case's map; every third case has one LONGER than the corpus (the rows behind `case.rows` belong to no corpus row)."""
    extra = (0, 0, 37)[case.seed % 3]
    return message_map(case.n_messages, case.rows + extra, case.layout, case.seed)


def accept_sets(n_messages: int, seed: int) -> dict[str, np.ndarray]:
    """The accept sets of a mask case: empty, every message, the first only, the last only, one with duplicates, one with entries below 0
    and at or beyond n_messages."""
    rng = np.random.default_rng(seed + 1)
    some = rng.choice(n_messages, size=max(1, n_messages // 3), replace=False).astype(np.int64)
    return {
        "empty": np.zeros(0, dtype=np.int64),
        "every": np.arange(n_messages, dtype=np.int64),
        "first": np.array([0], dtype=np.int64),
        "last": np.array([n_messages - 1], dtype=np.int64),
        "duplicates": np.concatenate([some, some[::-1], some[:1], some[:1]]),
        "out_of_range": np.concatenate([[-1, -5, n_messages, n_messages + 7, 2**31 - 2], some, [-(2**31)]]).astype(np.int64),
    }


def twin_mask_words(row_to_msg: np.ndarray, rows: int, accept: np.ndarray, n_bits: int) -> np.ndarray:
    """`mask_from_messages_kernel` in numpy: the accept bitmap over n_bits ordinals (entries outside it ignored); then, per round of 64 rows,
    lane l votes for row 64 g + l (no when the row is at or beyond `rows`, has no message, or its message is at or beyond n_bits or not in
    the bitmap) and the round's ballot is words 2 g and 2 g + 1 -> uint32 [(rows + 31) // 32], the bits at or beyond `rows` zero."""
    bitmap = np.zeros((n_bits + 31) // 32 + 1, dtype=np.uint32)
    acc = np.asarray(accept, dtype=np.int64)
    acc = acc[(acc >= 0) & (acc < n_bits)]
    np.bitwise_or.at(bitmap, acc >> 5, (np.uint32(1) << (acc & 31).astype(np.uint32)))
    groups = (rows + 63) // 64
    votes = np.zeros(groups * 64, dtype=bool)  # one per lane and round
    msg = np.asarray(row_to_msg[:rows], dtype=np.int64)
    live = (msg >= 0) & (msg < n_bits)
    m = np.where(live, msg, 0)
    votes[:rows] = live & (((bitmap[m >> 5] >> (m & 31).astype(np.uint32)) & 1) != 0)
    ballots = np.packbits(votes.reshape(groups, 64), axis=1, bitorder="little").view("<u8").reshape(groups)
    words = np.stack([(ballots & 0xFFFFFFFF).astype(np.uint32), (ballots >> np.uint64(32)).astype(np.uint32)], axis=1).reshape(-1)
    return words[: (rows + 31) // 32]


def isin_mask(row_to_msg: np.ndarray, rows: int, accept: np.ndarray) -> np.ndarray:
    """What `VectorBase.message_mask` is defined as: bool [rows]."""
    held = np.asarray(row_to_msg[:rows], dtype=np.int64)
    return np.isin(held, accept) & (held >= 0)


# ---- lookup cases ----------------------------------------------------------------------------------------------------------------------

ROWS = 3000
N_MESSAGES = 1000
MAX_QUERIES = 130


@dataclass(frozen=True)
class Corpus:
    name: str
    dim: int
    dtype: str  # "float16" / "float32"
    seed: int


CORPORA = (Corpus("fp16-d64", 64, "float16", 9501), Corpus("fp32-d64", 64, "float32", 9502), Corpus("fp16-d72", 72, "float16", 9503))

# (option "mask_tile", option "mask_wide") -> the route forced
ROUTES = {"list": (0, 0), "tile": (2, 0), "wide": (0, 2)}

UNIFORM_THRESHOLD = 0.55
PER_QUERY_THRESHOLDS = (0.0, 0.5, 0.58, 1.5)

# (queries, max_matches, scope, thresholds): every value of each appears at least once, with every corpus under every route
SHAPES = (
    (1, 1, "1%", "uniform"),
    (8, 10, "50%", "per_query"),
    (9, 64, "100%", "uniform"),
    (33, 65, "50%", "uniform"),
    (64, 256, "1%", "per_query"),
    (65, None, "50%", "uniform"),
    (130, 10, "100%", "per_query"),
    (65, 64, "0%", "uniform"),
    (130, 256, "rows", "uniform"),
    (33, 10, "rows", "per_query"),
)


@dataclass(frozen=True)
class LookupCase:
    corpus: Corpus
    route: str
    nq: int
    max_matches: int | None
    scope: str
    thresholds: str

    @property
    def name(self) -> str:
        return f"{self.corpus.name}-{self.route}-q{self.nq}-k{self.max_matches}-{self.scope.replace('%', 'pct')}-{self.thresholds}"


LOOKUP_CASES = [LookupCase(c, r, *shape) for c in CORPORA for r in ROUTES for shape in SHAPES]


def lookup_map() -> np.ndarray:
    """The row -> message map of the lookup corpora: 1000 messages of 1 to 5 chunks interleaved over 3000 rows, about a tenth of the rows -1."""
    return message_map(N_MESSAGES, ROWS, "interleaved", 9600)


def scope_messages(scope: str) -> np.ndarray:
    """The message ordinals of a scope given as a share of the messages."""
    rng = np.random.default_rng(9601)
    if scope == "0%":
        return np.zeros(0, dtype=np.int64)
    if scope == "100%":
        return np.arange(N_MESSAGES, dtype=np.int64)
    share = {"1%": 0.01, "50%": 0.5}[scope]
    return np.sort(rng.choice(N_MESSAGES, size=int(N_MESSAGES * share), replace=False)).astype(np.int64)


def arbitrary_rows_mask() -> np.ndarray:
    """bool [ROWS]: about 40 % of the rows whatever their message -- rows mapped to -1 included (asserted by the host test)."""
    return np.random.default_rng(9602).random(ROWS) < 0.4


def case_mask(case: LookupCase) -> np.ndarray:
    """bool [ROWS]: the rows the case searches."""
    if case.scope == "rows":
        return arbitrary_rows_mask()
    return isin_mask(lookup_map(), ROWS, scope_messages(case.scope))


def case_thresholds(case: LookupCase):
    if case.thresholds == "uniform":
        return UNIFORM_THRESHOLD
    return [PER_QUERY_THRESHOLDS[i % len(PER_QUERY_THRESHOLDS)] for i in range(case.nq)]


def tile_serves(corpus: Corpus, max_hits: int) -> bool:
    """The 32/64-query tile: 1 <= k <= 64 and rows of a multiple of 64 bytes."""
    return 1 <= max_hits <= 64 and (corpus.dim * (2 if corpus.dtype == "float16" else 4)) % 64 == 0


def wide_serves(corpus: Corpus, max_hits: int) -> bool:
    """The 128/256-query filter tile + rescoring: fp16 corpora (any width, through the padded copy), 1 <= k <= 256."""
    return corpus.dtype == "float16" and 1 <= max_hits <= 256


def expected_route(case: LookupCase) -> int:
    """`masked_route` after the case: the forced route where it serves the shape, else the row list."""
    k = 10 if case.max_matches is None else case.max_matches
    if case.route == "tile" and tile_serves(case.corpus, k):
        return 2
    if case.route == "wide" and wide_serves(case.corpus, k):
        return 3
    return 1
