"""Shared by the top-messages tests on device groups and row-sharded indexes: the case table (maps, masks, K, thresholds), a numpy statement
of the merge of top-messages lists, and a numpy statement of "every shard's own top K, then the merge".  No GPU, no library call."""

import numpy as np

FAILED = np.uint64(0xFFFFFFFFFFFFFFFF)
LOW = np.uint64(0xFFFFFFFF)

MAPS = ("chunks3", "interleaved", "interleaved_holes")
MASKS = ("none", "random_0.5", "random_0.01", "no_shard_1", "boundaries")
NQS = (1, 9, 17)
THRESHOLDS = ("zero", "per_query", "nothing")
THR_CYCLE = [0.0, 0.5, 0.6, 0.45, 1.5, -0.2, 0.55, 0.52]
INTERLEAVED_MESSAGES = 1000


def message_map(rows: int, kind: str) -> np.ndarray:
    """chunks3: contiguous messages of 3 chunks (they straddle any shard bound that is no multiple of 3); interleaved: row % n_messages --
    every message has a chunk on every shard; interleaved_holes: the same with 5 % of the rows at -1 (no message)."""
    r = np.arange(rows, dtype=np.int64)
    if kind == "chunks3":
        return r // 3
    m = r % min(INTERLEAVED_MESSAGES, max(rows, 1))
    if kind == "interleaved_holes":
        m = m.copy()
        m[np.random.default_rng(rows + 5).random(rows) < 0.05] = -1
    return m


def ks_for(n_messages: int):
    return (1, 10, 300, n_messages + 5)


def group_mask(kind: str, bounds):
    """None, or a bool mask over bounds[-1] rows (bounds: the shard bounds of a three-shard group)"""
    n = bounds[-1]
    if kind == "none":
        return None
    m = np.zeros(n, dtype=bool)
    if kind.startswith("random_"):
        m = np.random.default_rng(n + 11).random(n) < float(kind.split("_")[1])
        m[n // 2] = True
    elif kind == "no_shard_1":
        m = np.random.default_rng(n + 12).random(n) < 0.3
        m[bounds[1] : bounds[2]] = False
    elif kind == "boundaries":
        for b in bounds[1:-1]:
            m[b - 1] = m[b] = True
        m[0] = m[n - 1] = True
    return m


def thresholds(kind: str, nq: int):
    if kind == "zero":
        return 0.0
    if kind == "nothing":
        return 1.5
    return [THR_CYCLE[i % len(THR_CYCLE)] for i in range(nq)]


def threshold_of(kind: str, i: int) -> float:
    return {"zero": 0.0, "nothing": 1.5}.get(kind, THR_CYCLE[i % len(THR_CYCLE)])


def make_keys(scores, messages) -> np.ndarray:
    s = np.asarray(scores, dtype=np.float32)
    return (s.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (LOW - np.asarray(messages).astype(np.uint64))


def best_keys(keys: np.ndarray, k: int) -> np.ndarray:
    """any keys -> uint64 [k]: zeros dropped, per message (the low half) the largest key, sorted descending, cut at k, zero-padded"""
    keys = np.sort(keys[keys != 0])[::-1]
    _, first = np.unique(keys & LOW, return_index=True)  # in descending order a message's first key is its largest
    best = keys[np.sort(first)][:k]
    out = np.zeros(k, dtype=np.uint64)
    out[: len(best)] = best
    return out


def merge_statement(lists: np.ndarray) -> np.ndarray:
    """The merge of top-messages lists, stated in numpy: lists uint64 [n_lists, nq, k] -> [nq, k].  A query one of whose lists leads with
    the failure key is that key in every slot."""
    n_lists, nq, k = lists.shape
    out = np.zeros((nq, k), dtype=np.uint64)
    for q in range(nq):
        if (lists[:, q, 0] == FAILED).any():
            out[q] = FAILED
        else:
            out[q] = best_keys(lists[:, q, :].reshape(-1), k)
    return out


def collapse_keys(scores: np.ndarray, row_to_msg: np.ndarray, k: int, thr: float, allowed=None) -> np.ndarray:
    """The whole-corpus answer as keys [k]: rows with score >= thr (inside `allowed`, with a message) -> per message the best -> top k"""
    keep = (scores >= np.float32(thr)) & (row_to_msg >= 0)
    if allowed is not None:
        keep &= allowed
    return best_keys(make_keys(scores[keep], row_to_msg[keep]), k)


def shard_then_merge(scores: np.ndarray, row_to_msg: np.ndarray, k: int, thr: float, bounds, allowed=None) -> np.ndarray:
    """every shard's own top k over its rows, then the merge statement"""
    lists = np.zeros((len(bounds) - 1, 1, k), dtype=np.uint64)
    for g, (lo, hi) in enumerate(zip(bounds, bounds[1:])):
        lists[g, 0] = collapse_keys(scores[lo:hi], row_to_msg[lo:hi], k, thr, None if allowed is None else allowed[lo:hi])
    return merge_statement(lists)[0]


def random_lists(rng, n_lists: int, nq: int, k: int, fill: str, n_messages: int) -> np.ndarray:
    """uint64 [n_lists, nq, k]: sorted, zero-padded lists, one key per message within a list, messages shared between the lists.
    fill: "full" = min(k, n_messages) keys per list, "ragged" = 0 .. that many (one list empty), "empty" = none."""
    lists = np.zeros((n_lists, nq, k), dtype=np.uint64)
    if fill == "empty":
        return lists
    most = min(k, n_messages)
    grid = np.linspace(0.0, 1.0, 97, dtype=np.float32)  # few distinct scores: ties between messages and between lists
    for q in range(nq):
        lens = np.full(n_lists, most) if fill == "full" else rng.integers(0, most + 1, size=n_lists)
        if fill == "ragged":
            lens[rng.integers(0, n_lists)] = 0
        for l in range(n_lists):
            msgs = rng.choice(n_messages, size=int(lens[l]), replace=False)
            lists[l, q, : lens[l]] = np.sort(make_keys(rng.choice(grid, size=int(lens[l])), msgs))[::-1]
    return lists


def decoded(keys: np.ndarray):
    """keys [k] -> (message ordinals, score bits) of the real ones"""
    live = keys[keys != 0]
    return (LOW - (live & LOW)).astype(np.int64).tolist(), (live >> np.uint64(32)).astype(np.uint32).tolist()
