"""The case table of the row-insertion tests (tests/test_gpu_insert_rows.py runs it on the device, tests/test_insert_rows_host.py checks
that it is self-consistent): numpy only, no GPU.  A case is the row count AFTER the insertion, a row shape, where the new rows go (as the
`at` argument of np.insert, built from a pattern of holes in the new index space), the rows per pass of an in-place expansion
("compact_pass_rows"; 0 = the library's default) and the route: in place with spare capacity, out of place from an adopted tensor, out of
place because the capacity ran out."""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests.remove_rows_cases import AROUND_CHUNK, CHUNK, NARROW_SHAPES, ODD_PASS, SMALL_SHAPES, TILE, WIDE_SHAPES, base_matrix, effective_pass, removed_flags

ROWS = (1, 2, 31, 32, 33, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17)  # rows after the insertion
# the hole patterns the removal table has (there: the rows that go; here: the rows that come), and two that only an `at` list can say
FLAG_KINDS = ("none", "first", "last", "all", "all_but_first", "all_but_last", "every_other", "block_in_chunk", "block_over_chunk_edge",
              "block_longer_than_pass", "random_1", "random_50", "random_99")
KINDS = FLAG_KINDS + ("repeated_at", "unsorted_at")
ROUTES = ("in_place", "adopted", "no_capacity")
PASSES = (0, CHUNK, 64, ODD_PASS)


@dataclass(frozen=True)
class Case:
    rows: int  # after the insertion
    dim: int
    dtype: str
    kind: str
    pass_rows: int
    route: str

    @property
    def id(self) -> str:
        return f"{self.rows}x{self.dim}{self.dtype}-{self.kind}-pass{self.pass_rows}-{self.route}"


def positions_of(at: np.ndarray, n_old: int) -> np.ndarray:
    """The documented rule (numpy's own): wrap the negatives, stable argsort, `+= arange(m)` -> where value row j stands afterwards."""
    idx = np.array(at, dtype=np.int64).reshape(-1)
    assert ((idx >= -n_old) & (idx <= n_old)).all()
    idx[idx < 0] += n_old
    order = idx.argsort(kind="stable")
    idx[order] += np.arange(len(idx), dtype=np.int64)
    return idx


def insertion(kind: str, rows: int, pass_rows: int) -> np.ndarray | None:
    """int64 [m]: the `at` argument that leaves `rows` rows; None where the kind does not exist at this size."""
    if kind == "repeated_at":  # many rows in front of ONE old row
        if rows < 3:
            return None
        m = max(1, rows // 3)
        return np.full(m, (rows - m) // 2, dtype=np.int64)
    if kind == "unsorted_at":  # positions in no order, some of them equal, some negative
        if rows < 4:
            return None
        m = max(2, rows // 4)
        rng = np.random.default_rng(77 + rows)
        at = rng.integers(0, rows - m + 1, size=m)
        at[m // 2 :] = at[: m - m // 2]  # every position of the first half again: equal positions keep their order
        rng.shuffle(at)
        third = np.zeros(m, dtype=bool)
        third[::3] = True
        at[third & (at < rows - m)] -= rows - m  # the same positions, counted from the end (the old length itself has no such form)
        if (np.diff(positions_of(at, rows - m)) >= 0).all():
            return None
        return at.astype(np.int64)
    f = removed_flags(kind, rows, pass_rows)
    if f is None:
        return None
    p = np.flatnonzero(f)
    return (p - np.arange(len(p))).astype(np.int64)  # hole j stands in front of old row p[j] - j


@lru_cache(maxsize=1)
def cases() -> tuple[Case, ...]:
    out: list[Case] = []
    seen = set()

    def add(rows, shape, kind, pass_rows, route):
        dim, dtype = shape
        pr = pass_rows if route == "in_place" else 0
        if insertion(kind, rows, effective_pass(pr, dim, dtype)) is None:
            return
        c = Case(rows, dim, dtype, kind, pr, route)
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    # every (rows, kind) pair once, the shape, the route and the pass size taking turns
    turn = 0
    for i, rows in enumerate(ROWS):
        for j, kind in enumerate(KINDS):
            if kind == "block_longer_than_pass":
                continue  # (below, where the pass is short enough)
            shape = SMALL_SHAPES[(i + j) % 3]
            route = ROUTES[(i + 2 * j) % 3]
            pass_rows = (0, CHUNK, 64)[turn % 3]
            if pass_rows == 64 and rows > CHUNK + 1:
                pass_rows = CHUNK
            add(rows, shape, kind, pass_rows, route)
            turn += 1
    # a block longer than a pass, and many passes, at sizes where that stays quick
    for rows, pass_rows in ((CHUNK - 1, 64), (CHUNK + 1, 64), (CHUNK + 1, ODD_PASS), (2 * CHUNK + 17, ODD_PASS), (2 * CHUNK + 17, CHUNK)):
        for shape in SMALL_SHAPES:
            add(rows, shape, "block_longer_than_pass", pass_rows, "in_place")
    for kind in ("first", "every_other", "random_50", "all_but_last", "repeated_at", "unsorted_at"):
        add(CHUNK + 1, SMALL_SHAPES[1], kind, 64, "in_place")
        add(2 * CHUNK + 17, SMALL_SHAPES[0], kind, ODD_PASS, "in_place")
    for rows in (33, 64, 65):
        for kind in ("first", "every_other", "random_50", "unsorted_at"):
            add(rows, SMALL_SHAPES[2], kind, 64, "in_place")
    # every route at the kind that exists at two sizes only
    for t, route in enumerate(ROUTES):
        add(CHUNK + 1, SMALL_SHAPES[t], "block_over_chunk_edge", 0, route)
    # the model widths around one chunk
    for i, rows in enumerate(AROUND_CHUNK):
        for j, shape in enumerate(WIDE_SHAPES):
            for t, kind in enumerate(("first", "last", "random_1", "random_50", "every_other", "block_over_chunk_edge", "repeated_at", "unsorted_at")[(i + j) % 2 :: 2]):
                add(rows, shape, kind, (0, 4096)[(i + j + t) % 2], ROUTES[(j + t) % 3])
    # the narrowest copies
    for shape in NARROW_SHAPES:
        for rows in (33, CHUNK + 1):
            for kind, route in (("every_other", "in_place"), ("random_50", "adopted"), ("first", "in_place"), ("unsorted_at", "no_capacity")):
                add(rows, shape, kind, 0, route)
    return tuple(out)


def at(case: Case) -> np.ndarray:
    a = insertion(case.kind, case.rows, effective_pass(case.pass_rows, case.dim, case.dtype))
    assert a is not None
    return a


def old_matrix(case: Case) -> np.ndarray:
    """float32 [rows before the insertion, dim], every value exact in fp16."""
    return base_matrix(case.dim)[: case.rows - len(at(case))]


def new_matrix(case: Case) -> np.ndarray:
    """float32 [m, dim]: the rows that come, exact in fp16 and unlike every old row (the old rows' second column is never negative)."""
    m = -base_matrix(case.dim)[: len(at(case))]
    m[:, 1] -= 1.0
    return m


def holes(case: Case) -> np.ndarray:
    """bool [rows]: the new rows, in the new index space."""
    a = at(case)
    f = np.zeros(case.rows, dtype=bool)
    f[positions_of(a, case.rows - len(a))] = True
    return f
