"""The case table of the row-removal tests (tests/test_gpu_remove_rows.py runs it on the device, tests/test_remove_rows_host.py checks that
it is self-consistent): numpy only, no GPU.  A case is a corpus shape, a set of rows to remove, the rows per pass of an in-place
compaction ("compact_pass_rows"; 0 = the library's default) and the route (in place, or out of place from an adopted tensor)."""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np

CHUNK = 16384  # TAVB_MASK_ROWS_PER_WORKGROUP: the per-chunk counts the kernels find their slots by
TILE = 64  # rows one workgroup of the gather takes; passes are whole tiles
ROWS = (1, 2, 31, 32, 33, 64, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 17)
AROUND_CHUNK = (CHUNK - 1, CHUNK, CHUNK + 1)
# (dim, dtype): 16-byte rows; rows that are 8- but not 16-byte aligned; fp32; the model widths
SMALL_SHAPES = ((8, "f16"), (100, "f16"), (100, "f32"))
WIDE_SHAPES = ((384, "f16"), (384, "f32"), (1536, "f16"), (1536, "f32"))
# rows that are only 2-byte (33 halves) and only 4-byte (33 floats) aligned: the narrowest copies
NARROW_SHAPES = ((33, "f16"), (33, "f32"))
ODD_PASS = 4160  # 65 tiles: does not divide a chunk
KINDS = ("none", "first", "last", "all", "all_but_first", "all_but_last", "every_other", "block_in_chunk", "block_over_chunk_edge",
         "block_longer_than_pass", "random_1", "random_50", "random_99")
ROUTES = ("in_place", "out_of_place")


@dataclass(frozen=True)
class Case:
    rows: int
    dim: int
    dtype: str
    kind: str
    pass_rows: int
    route: str

    @property
    def id(self) -> str:
        return f"{self.rows}x{self.dim}{self.dtype}-{self.kind}-pass{self.pass_rows}-{self.route}"


def effective_pass(pass_rows: int, dim: int, dtype: str) -> int:
    """Rows per pass as the library cuts them: the option rounded up to whole tiles; 0 = about 64 MiB of rows."""
    if pass_rows <= 0:
        pass_rows = max((64 << 20) // (dim * (2 if dtype == "f16" else 4)), 1)
    return (pass_rows + TILE - 1) // TILE * TILE


def removed_flags(kind: str, rows: int, pass_rows: int) -> np.ndarray | None:
    """bool [rows]: the rows the case removes; None where the kind does not exist at this size."""
    f = np.zeros(rows, dtype=bool)
    if kind == "none":
        return f
    if kind == "first":
        f[0] = True
    elif kind == "last":
        f[-1] = True
    elif kind == "all":
        f[:] = True
    elif kind == "all_but_first":
        if rows < 2:
            return None
        f[1:] = True
    elif kind == "all_but_last":
        if rows < 2:
            return None
        f[:-1] = True
    elif kind == "every_other":
        if rows < 2:
            return None
        f[1::2] = True
    elif kind == "block_in_chunk":
        if rows < 8:
            return None
        f[rows // 4 : min(rows // 2, CHUNK)] = True
    elif kind == "block_over_chunk_edge":
        if rows <= CHUNK:
            return None
        f[CHUNK - 100 : min(CHUNK + 100, rows)] = True
    elif kind == "block_longer_than_pass":
        if rows < pass_rows + 3 * TILE:
            return None
        f[TILE // 2 : TILE // 2 + pass_rows + TILE + 5] = True
    else:
        pct = int(kind.split("_")[1])
        rng = np.random.default_rng(1000 * pct + rows)
        n = max(1, rows * pct // 100) if rows * pct >= 100 or pct == 50 else 0
        if n == 0 or n > rows:
            return None
        f[rng.choice(rows, size=n, replace=False)] = True
    return f


@lru_cache(maxsize=1)
def cases() -> tuple[Case, ...]:
    out: list[Case] = []
    seen = set()

    def add(rows, shape, kind, pass_rows, route):
        dim, dtype = shape
        pr = pass_rows if route == "in_place" else 0
        if removed_flags(kind, rows, effective_pass(pr, dim, dtype)) is None:
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
            route = ROUTES[(i + j) % 2]
            pass_rows = (0, CHUNK, 64)[turn % 3]
            if pass_rows == 64 and rows > CHUNK + 1:
                pass_rows = CHUNK
            add(rows, shape, kind, pass_rows, route)
            turn += 1
    # a block longer than a pass, and many passes, at sizes where that stays quick
    for rows, pass_rows in ((CHUNK - 1, 64), (CHUNK + 1, 64), (CHUNK + 1, ODD_PASS), (2 * CHUNK + 17, ODD_PASS), (2 * CHUNK + 17, CHUNK)):
        for shape in SMALL_SHAPES:
            add(rows, shape, "block_longer_than_pass", pass_rows, "in_place")
    for kind in ("first", "every_other", "random_50", "all_but_last"):
        add(CHUNK + 1, SMALL_SHAPES[1], kind, 64, "in_place")
        add(2 * CHUNK + 17, SMALL_SHAPES[0], kind, ODD_PASS, "in_place")
    for rows in (33, 64):
        for kind in ("first", "every_other", "random_50"):
            add(rows, SMALL_SHAPES[2], kind, 64, "in_place")
    # the model widths around one chunk
    for i, rows in enumerate(AROUND_CHUNK):
        for j, shape in enumerate(WIDE_SHAPES):
            for t, kind in enumerate(("first", "last", "random_1", "random_50", "every_other", "block_over_chunk_edge")[(i + j) % 2 :: 2]):
                add(rows, shape, kind, (0, 4096)[(i + j + t) % 2], ROUTES[(j + t) % 2])
    # the narrowest copies
    for shape in NARROW_SHAPES:
        for rows in (33, CHUNK + 1):
            for kind, route in (("every_other", "in_place"), ("random_50", "out_of_place"), ("first", "in_place")):
                add(rows, shape, kind, 0, route)
    return tuple(out)


@lru_cache(maxsize=None)
def base_matrix(dim: int) -> np.ndarray:
    """float32 [most rows of the table, dim]: a case takes its first `rows` rows.  Every value is exact in fp16, and no two rows are equal."""
    rows = max(ROWS) if dim <= 384 else max(AROUND_CHUNK)
    rng = np.random.default_rng(dim)
    m = rng.integers(-1024, 1025, size=(rows, dim)).astype(np.float32) / 1024.0
    m[:, 0] = (np.arange(rows) % 2048).astype(np.float32) / 2048.0  # with the next column: the row's number
    m[:, 1] = (np.arange(rows) // 2048).astype(np.float32)
    m.setflags(write=False)
    return m


def matrix(case: Case) -> np.ndarray:
    return base_matrix(case.dim)[: case.rows]


def flags(case: Case) -> np.ndarray:
    f = removed_flags(case.kind, case.rows, effective_pass(case.pass_rows, case.dim, case.dtype))
    assert f is not None
    return f
