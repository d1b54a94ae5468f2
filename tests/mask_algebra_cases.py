"""TEST INFRASTRUCTURE -- the case table of the scope algebra, shared by tests/test_gpu_mask_algebra.py (the device) and
tests/test_mask_algebra_host.py (its CPU twin, which pins the table's own claims against brute-force numpy).

Combine cases: every row count of `ROWS` x op x operand count x the kind of operand 0 (the other operands are random masks of density
0.7, so that an AND of eight is not trivially empty).  `twin_combine_words` restates `mask_combine_kernel` in numpy: every operand word
read through `mask_word` (the bits at or beyond `rows` dropped), the op, the complement cut at `rows`.

Range cases: `scopes(rows)` -- named scopes of 0, 1, 2 and 8 collections built from the range sets the kernel can go wrong on.
`merge_collection` restates the host's sort / clip / merge in plain Python, `twin_range_words` the kernel: rounds of 64 rows, one binary
search per collection and lane, two words per ballot."""

from __future__ import annotations

import numpy as np

C = 16384  # _native.MASK_ROWS_PER_WORKGROUP (asserted by the host test)
LDS_RANGES = 1024  # _native.SCOPE_LDS_RANGES (asserted by the host test)
ROWS = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, C - 1, C, C + 1, 3 * C + 17)
AND, OR, ANDNOT = 0, 1, 2
OPS = {"and": AND, "or": OR, "andnot": ANDNOT}
OPERAND_COUNTS = (1, 2, 3, 8)
KINDS = ("none", "all", "first", "last", "alternating", "random0.01", "random0.5", "last_word")


def operand(kind: str, rows: int, seed: int) -> np.ndarray:
    """bool [rows]: one operand of a combine case."""
    m = np.zeros(rows, dtype=bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind.startswith("random"):
        m = np.random.default_rng(seed).random(rows) < float(kind[len("random"):])
    elif kind == "last_word":
        m[(rows - 1) // 32 * 32:] = True
    elif kind != "none":
        raise ValueError(kind)
    return m


def operands(kind: str, n: int, rows: int) -> list[np.ndarray]:
    """The n operands of a combine case: operand 0 of `kind`, the others random masks of density 0.7."""
    seed = 7000 + 31 * KINDS.index(kind) + rows % 1009
    return [operand(kind, rows, seed)] + [operand("random0.7", rows, seed + 1 + j) for j in range(n - 1)]


def combine_bools(op: int, ms: list[np.ndarray]) -> np.ndarray:
    """Brute force: what the combination is defined as, on bool arrays."""
    if op == AND:
        return np.logical_and.reduce(ms)
    if op == OR:
        return np.logical_or.reduce(ms)
    return ~ms[0] if len(ms) == 1 else ms[0] & ~np.logical_or.reduce(ms[1:])


def pack(mask: np.ndarray, dirty: bool = False) -> np.ndarray:
    """bool [rows] -> uint32 [(rows + 31) // 32 + 1]: the packed mask (row r = bit r & 31 of word r >> 5) and one word BEHIND it.  dirty:
    every bit at or beyond `rows` set, the word behind all ones -- what the kernels must ignore."""
    rows = len(mask)
    n_words = (rows + 31) // 32
    bits = np.zeros((n_words + 1) * 32, dtype=bool)
    bits[:rows] = mask
    if dirty:
        bits[rows:] = True
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def twin_combine_words(op: int, words: list[np.ndarray], rows: int) -> np.ndarray:
    """`mask_combine_kernel` in numpy over packed operands (which may be dirty): uint32 [(rows + 31) // 32], tail bits zero."""
    n_words = (rows + 31) // 32
    tail = rows & 31
    keep = np.full(n_words, 0xFFFFFFFF, dtype=np.uint32)
    if tail:
        keep[-1] = (1 << tail) - 1
    clean = [np.asarray(w[:n_words], dtype=np.uint32) & keep for w in words]  # mask_word
    v = clean[0].copy()
    rest = np.zeros(n_words, dtype=np.uint32)
    for t in clean[1:]:
        if op == AND:
            v &= t
        elif op == OR:
            v |= t
        else:
            rest |= t
    if op == ANDNOT:
        v = (~v if len(clean) == 1 else v & ~rest) & keep
    return v


# ---- ranges ------------------------------------------------------------------------------------------------------------------------------

def merge_collection(ranges, n: int) -> list[tuple[int, int]]:
    """The host's preparation of one collection: clipped to [0, n), empties dropped, sorted, overlapping and touching ranges merged."""
    kept = sorted((max(int(s), 0), min(int(e), n)) for s, e in ranges if max(int(s), 0) < min(int(e), n))
    out: list[tuple[int, int]] = []
    for s, e in kept:
        if out and s <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], e))
        else:
            out.append((s, e))
    return out


def range_bool(collections, rows: int, row_to_msg=None) -> np.ndarray:
    """Brute force: bool [rows], row r set when every collection has a range that holds x = r (row_to_msg None) or x = row_to_msg[r] (never
    when that is below 0)."""
    x = np.arange(rows, dtype=np.int64) if row_to_msg is None else np.asarray(row_to_msg[:rows], dtype=np.int64)
    ok = x >= 0
    for col in collections:
        hit = np.zeros(rows, dtype=bool)
        for s, e in col:
            hit |= (x >= int(s)) & (x < int(e))
        ok &= hit
    return ok


def twin_range_words(collections, rows: int, row_to_msg=None, n_messages: int = 0) -> np.ndarray:
    """`mask_from_ranges_kernel` in numpy: the merged intervals of every collection; per round of 64 rows lane l votes for row 64 g + l -- no
    when it is at or beyond `rows`, when its message is outside [0, n_messages), or when a collection's binary search (the number of
    intervals that start at or before x, then x < the end of the last of them) fails -- and the ballot is words 2 g and 2 g + 1."""
    n = rows if row_to_msg is None else n_messages
    groups = (rows + 63) // 64
    votes = np.zeros(groups * 64, dtype=bool)
    x = np.arange(rows, dtype=np.int64) if row_to_msg is None else np.asarray(row_to_msg[:rows], dtype=np.int64)
    on = np.ones(rows, dtype=bool) if row_to_msg is None else (x >= 0) & (x < n_messages)
    for col in collections:
        iv = np.asarray(merge_collection(col, n), dtype=np.int64).reshape(-1, 2)
        lo = np.searchsorted(iv[:, 0], x, side="right")
        on &= (lo > 0) & (x < iv[np.maximum(lo, 1) - 1, 1] if len(iv) else False)
    votes[:rows] = on
    ballots = np.packbits(votes.reshape(groups, 64), axis=1, bitorder="little").view("<u8").reshape(groups)
    words = np.stack([(ballots & 0xFFFFFFFF).astype(np.uint32), (ballots >> np.uint64(32)).astype(np.uint32)], axis=1).reshape(-1)
    return words[: (rows + 31) // 32]


def range_sets(rows: int) -> dict[str, list[tuple[int, int]]]:
    """The single collections the scopes are built from."""
    rng = np.random.default_rng(8100 + rows % 1013)
    starts = rng.integers(-5, rows + 5, size=40)
    some = [(int(s), int(s + w)) for s, w in zip(starts, rng.integers(-2, max(rows // 8, 3), size=40))]
    sets = {
        "everything": [(0, rows)],
        "duplicates": [some[i] for i in rng.permutation(40)] + some[:10] + some[5:15][::-1],  # unsorted, overlapping, repeated, some empty
        "empty": [],
        "only_empties": [(5, 5), (9, 3), (rows, rows + 4), (-7, 0)],
        "outside": [(-10, (rows + 1) // 2), (rows - 3, rows + 100)],
    }
    for b in (32, 64, C):  # one range ending at a word, wave and chunk boundary and one past it
        sets[f"end{b}"] = [(0, b)]
        sets[f"end{b}+1"] = [(0, b + 1)]
    return sets


def scopes(rows: int) -> dict[str, list[list[tuple[int, int]]]]:
    """name -> the collections of a scope: none, every single set, pairs, eight, an empty collection among full ones, and totals of exactly
    LDS_RANGES merged intervals and one more (in one collection and across two) where the rows hold that many."""
    s = range_sets(rows)
    out: dict[str, list] = {"no_collection": []}
    for name, col in s.items():
        out[f"1:{name}"] = [col]
    out["2:duplicates+outside"] = [s["duplicates"], s["outside"]]
    out["2:end64+1+duplicates"] = [s["end64+1"], s["duplicates"]]
    out["2:everything+empty"] = [s["everything"], s["empty"]]
    out["8:mixed"] = [s["everything"], s["duplicates"], s["outside"], s[f"end{C}+1"], s["everything"], s["duplicates"][::-1], s[f"end{C}"], s["outside"]]
    out["8:empty_among_full"] = [s["everything"]] * 5 + [s["only_empties"]] + [s["everything"]] * 2
    out["8:full"] = [s["everything"]] * 8
    if rows >= 2 * LDS_RANGES + 1:
        singles = [(2 * i, 2 * i + 1) for i in range(LDS_RANGES + 1)]  # never touching: nothing merges
        out["lds:exact"] = [singles[:LDS_RANGES]]
        out["lds:one_more"] = [singles]
        out["lds:exact_in_two"] = [singles[: LDS_RANGES // 2], singles[: LDS_RANGES // 2]]
        out["lds:one_more_in_two"] = [singles[: LDS_RANGES // 2], singles[: LDS_RANGES // 2 + 1]]
    return out


def merged_total(collections, n: int) -> int:
    return sum(len(merge_collection(c, n)) for c in collections)


def message_scopes(n_messages: int, seed: int) -> dict[str, list[list[tuple[int, int]]]]:
    """Scopes over message ordinals for the maps of tests/message_scope_cases.py."""
    rng = np.random.default_rng(seed + 2)
    cuts = sorted(int(v) for v in rng.integers(0, n_messages + 1, size=6))
    return {
        "no_collection": [],
        "everything": [[(0, n_messages)]],
        "beyond": [[(-4, n_messages + 9)]],
        "first": [[(0, 1)]],
        "last": [[(n_messages - 1, n_messages)]],
        "pieces": [[(cuts[0], cuts[1]), (cuts[4], cuts[5]), (cuts[2], cuts[3]), (cuts[2], cuts[3])]],
        "two": [[(cuts[0], cuts[3])], [(cuts[1], cuts[5]), (cuts[0], cuts[0])]],
        "empty_collection": [[(0, n_messages)], []],
    }
