"""The case table of the carried-mask tests (tests/test_gpu_mask_carry.py runs it on the device, tests/test_mask_carry_host.py checks that
it is self-consistent and runs the host fallback over it): numpy only, no GPU.  A case is one row edit -- a removal, an insertion or an
append -- of an index of `rows` rows, the masks carried through it and whether the new rows are set.  The row counts are the word and
chunk edges of tavb_mask_remap (32 rows a word, 16384 rows a chunk); `expected` is numpy's own delete / insert / concatenate."""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import remove_rows_cases as rc
from tests.insert_rows_cases import positions_of

CHUNK = rc.CHUNK
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17)  # rows BEFORE the edit
AROUND_CHUNK = (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17)
DIM = 64
DTYPES = ("fp16", "fp32")
REMOVE_KINDS = rc.KINDS + ("whole_word",)
INSERT_KINDS = ("front", "middle", "at_len", "scattered", "block_over_chunk_edge", "outgrow")
APPEND_KINDS = ("by_1", "by_31", "by_32", "over_chunk_edge")
MASK_KINDS = ("empty", "all", "removal", "complement", "last", "first", "random_1", "random_50")
MASK_COUNTS = (1, 8, 9, 17)
_PASS = 64  # what "block_longer_than_pass" of the removal kinds is cut by here


@dataclass(frozen=True)
class Case:
    mode: str  # "remove", "insert" or "append"
    rows: int
    kind: str
    n_masks: int
    fill: bool  # carry_new= / new=
    dtype: str

    @property
    def id(self) -> str:
        return f"{self.mode}-{self.rows}-{self.kind}-{self.n_masks}masks-{'set' if self.fill else 'clear'}-{self.dtype}"


def removal(kind: str, rows: int) -> np.ndarray | None:
    """bool [rows]: the rows a removal of this kind takes; None where the kind does not exist at this size."""
    if kind == "whole_word":  # exactly the second word of the mask: the pieces behind it move down by a whole word
        if rows < 64:
            return None
        f = np.zeros(rows, dtype=bool)
        f[32:64] = True
        return f
    return rc.removed_flags(kind, rows, _PASS)


def insertion(kind: str, rows: int):
    """(at, m): the `at` argument of an insertion of m rows into `rows` rows; None where the kind does not exist at this size."""
    if kind == "front":
        return 0, 1
    if kind == "middle":
        return (rows // 2, 1) if rows >= 2 else None
    if kind == "at_len":
        return rows, 1
    if kind == "scattered":  # positions in no order, equal ones among them, the ends included
        if rows < 2:
            return None
        m = max(4, rows // 16)
        rng = np.random.default_rng(300 + rows)
        at = rng.integers(0, rows + 1, size=m)
        at[1] = at[0]
        at[-1] = rows
        at[-2] = 0
        return at.astype(np.int64), m
    if kind == "block_over_chunk_edge":  # new rows [CHUNK - 50, CHUNK + 50)
        return (CHUNK - 50, 100) if rows >= CHUNK - 1 else None
    if kind == "outgrow":  # more than doubles the index: no growth buffer holds it, the rows move to a new one
        return rows // 3, rows + 20
    raise ValueError(kind)


def appended(kind: str, rows: int) -> int | None:
    if kind == "over_chunk_edge":
        return CHUNK - rows % CHUNK + 3 if rows >= CHUNK - 1 else None
    return int(kind.split("_")[1])


@lru_cache(maxsize=1)
def cases() -> tuple[Case, ...]:
    out: list[Case] = []
    turn = 0

    def add(mode, rows, kind, n_masks=None, fill=None):
        nonlocal turn
        out.append(Case(mode, rows, kind, MASK_COUNTS[turn % 4] if n_masks is None else n_masks, bool(turn % 2) if fill is None else fill,
                        DTYPES[(turn // 2) % 2]))
        turn += 1

    for rows in ROWS:
        for kind in REMOVE_KINDS:
            if removal(kind, rows) is not None:
                add("remove", rows, kind, fill=False)
        for kind in INSERT_KINDS:
            if insertion(kind, rows) is not None:
                add("insert", rows, kind)
                if rows in AROUND_CHUNK:  # `carry_new` both ways where the kernel has more than one workgroup
                    add("insert", rows, kind, fill=not out[-1].fill)
        for kind in APPEND_KINDS:
            if appended(kind, rows) is not None:
                add("append", rows, kind)
                if rows in AROUND_CHUNK or rows in (31, 32, 33):
                    add("append", rows, kind, fill=not out[-1].fill)
    # every number of handles at the largest size of every mode, both fills
    for n_masks in MASK_COUNTS:
        add("remove", 2 * CHUNK + 17, "random_50", n_masks, False)
        for fill in (False, True):
            add("insert", 2 * CHUNK + 17, "scattered", n_masks, fill)
            add("append", 2 * CHUNK + 17, "by_31", n_masks, fill)
    seen, unique = set(), []
    for c in out:
        if c.id not in seen:
            seen.add(c.id)
            unique.append(c)
    return tuple(unique)


def flags(case: Case) -> np.ndarray:
    """The edit's flags as the device reads them: remove -- bool [rows], set = the row goes; insert -- bool [rows + m], set = a hole."""
    if case.mode == "remove":
        return removal(case.kind, case.rows)
    assert case.mode == "insert"
    at, m = insertion(case.kind, case.rows)
    pos = positions_of(np.full(m, at) if np.ndim(at) == 0 else at, case.rows)
    f = np.zeros(case.rows + m, dtype=bool)
    f[pos] = True
    return f


def new_rows(case: Case) -> int:
    if case.mode == "remove":
        return case.rows - int(removal(case.kind, case.rows).sum())
    if case.mode == "insert":
        return case.rows + insertion(case.kind, case.rows)[1]
    return case.rows + appended(case.kind, case.rows)


def masks(case: Case) -> list[np.ndarray]:
    """The carried masks, bool [rows] each: the kinds of MASK_KINDS in turn (one handle: the densest random one)."""
    n = case.rows
    base = removal(case.kind, n) if case.mode == "remove" else np.arange(n) % 2 == 1
    kinds = ("random_50",) if case.n_masks == 1 else MASK_KINDS
    out = []
    for i in range(case.n_masks):
        kind = kinds[i % len(kinds)]
        b = np.zeros(n, dtype=bool)
        if kind == "all":
            b[:] = True
        elif kind == "removal":
            b = base.copy()
        elif kind == "complement":
            b = ~base
        elif kind == "last":
            b[-1] = True
        elif kind == "first":
            b[0] = True
        elif kind.startswith("random"):
            pct = int(kind.split("_")[1])
            b = np.random.default_rng(17 * n + 1000 * i + pct).random(n) * 100 < pct
        out.append(b)
    return out


def expected(case: Case) -> list[np.ndarray]:
    """numpy's answer: what every carried mask must equal after the edit."""
    if case.mode == "remove":
        which = np.flatnonzero(removal(case.kind, case.rows))
        return [np.delete(b, which) for b in masks(case)]
    if case.mode == "insert":
        at, _ = insertion(case.kind, case.rows)
        if np.ndim(at) == 0:  # one position, m rows: np.insert takes the values' length from the values
            m = insertion(case.kind, case.rows)[1]
            return [np.insert(b, at, np.full(m, case.fill)) for b in masks(case)]
        return [np.insert(b, at, case.fill) for b in masks(case)]
    return [np.concatenate([b, np.full(appended(case.kind, case.rows), case.fill)]) for b in masks(case)]


@lru_cache(maxsize=None)
def base_matrix() -> np.ndarray:
    """float32 [the most rows any case holds after its edit, DIM]: exact in fp16, no two rows equal (remove_rows_cases' recipe)."""
    rows = 2 * (2 * CHUNK + 17) + 20
    rng = np.random.default_rng(DIM + 24)
    m = rng.integers(-1024, 1025, size=(rows, DIM)).astype(np.float32) / 1024.0
    m[:, 0] = (np.arange(rows) % 2048).astype(np.float32) / 2048.0
    m[:, 1] = (np.arange(rows) // 2048).astype(np.float32) / 64.0
    m.setflags(write=False)
    return m


def old_matrix(case: Case) -> np.ndarray:
    return base_matrix()[: case.rows]


def new_vectors(case: Case) -> np.ndarray:
    """The rows an insertion or an append adds: taken from the far end of the base matrix."""
    m = new_rows(case) - case.rows
    return base_matrix()[::-1][:m]
