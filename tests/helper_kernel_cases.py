"""The case table of tests/test_gpu_helper_kernels.py and of its CPU twin tests/test_helper_kernel_cases_host.py: the small kernels of
csrc/tavb_misc.hip around the scan -- the merge of per-rank lists, L2 row normalisation, f32 -> f16 conversion and the load path that
rides it, the position remap of the sharded subset forms and the message re-rank -- on every branch each of them has.

Every kind of case carries its inputs, a plain numpy reference of the operation (float64 where rounding is at stake, uint64 arithmetic
for keys) and a small classifier that restates, from the launch code, WHICH branch of the kernel a case takes; the CPU twin asserts that
every branch has a case and that the references are right where there is something to check, the GPU file runs the kernels.

A plain module (no test, no fixture): both test files import it.
"""

from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests.synth import make_corpus

U32 = np.uint64(0xFFFFFFFF)
HI = np.uint64(0xFFFFFFFF00000000)
FAILED = np.uint64(0xFFFFFFFFFFFFFFFF)  # TAVB_KEY_PEER_FAILED


def pack_keys(scores: np.ndarray, ordinals: np.ndarray) -> np.ndarray:
    """(float32 scores, ordinals) -> uint64 keys (score bits << 32) | (0xFFFFFFFF - ordinal)"""
    bits = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (U32 - np.asarray(ordinals).astype(np.uint64))


# ---- 1. merge ----------------------------------------------------------------------------------------------------------------------------

MERGE_COUNTS = (1, 2, 3, 5, 8, 16, 17, 33, 48, 49, 64, 65, 100)
MERGE_KS = (1, 2, 63, 64, 65, 128, 200, 255, 256)
MERGE_FILLS = ("full", "ragged", "ties", "high", "one", "failed")


@dataclass(frozen=True)
class MergeCase:
    name: str
    n_lists: int
    k: int
    nq: int
    fill: str  # "full"; "ragged" (0 .. k keys per list, one list of every query empty, the last query of three wholly empty); "ties" (two
    #            distinct score bits: the ordinal half decides); "high" (ordinals counted down from 2^32 - 2); "one" (every list but one
    #            empty); "failed" (full, and one list of query 1 holds the failure key in every slot)
    seed: int


def _merge_cases():
    out = []

    def add(n, k, nq, fill):
        out.append(MergeCase(f"merge-n{n}-k{k}-q{nq}-{fill}", n, k, nq, fill, 7000 + 1000 * n + k))

    spread = {1: (1, 64, 65, 256), 2: (2, 63, 128, 255), 5: (1, 64, 200, 256), 16: (2, 63, 65, 255), 33: (1, 64, 128, 256),
              48: (2, 64, 65, 200), 49: (1, 63, 64, 256), 64: (2, 64, 65, 255), 65: (1, 63, 128, 256), 100: (2, 64, 200, 256)}
    i = 0
    for n in MERGE_COUNTS:
        for k in (MERGE_KS if n in (3, 8, 17) else spread[n]):
            add(n, k, (1, 3)[i % 2], ("full", "ragged")[i % 2])
            add_swapped = n in (3, 8, 17) and k in (64, 65)  # the edge of the two kernel forms in the other fill as well
            if add_swapped:
                add(n, k, (3, 1)[i % 2], ("ragged", "full")[i % 2])
            i += 1
    for n, k in ((3, 64), (8, 256), (17, 65), (49, 64), (100, 200)):
        for fill in ("ties", "high", "one"):
            add(n, k, 3, fill)
    add(8, 200, 3, "failed")
    add(49, 64, 3, "failed")
    return out


MERGE_CASES = _merge_cases()


def merge_lists(case: MergeCase) -> np.ndarray:
    """uint64 [n_lists, nq, k]: sorted (descending), zero-padded lists; the keys of a query are unique (but for the failure key)"""
    rng = np.random.default_rng(case.seed)
    n, nq, k = case.n_lists, case.nq, case.k
    lists = np.zeros((n, nq, k), dtype=np.uint64)
    for q in range(nq):
        lens = np.full(n, k)
        if case.fill == "ragged":
            lens = rng.integers(0, k + 1, size=n)
            lens[rng.integers(0, n)] = 0
            if nq > 1 and q == nq - 1:
                lens[:] = 0
        elif case.fill == "one":
            lens[:] = 0
            lens[rng.integers(0, n)] = k
        total = int(lens.sum())
        levels = np.linspace(0.0, 1.0, 97, dtype=np.float32)  # few distinct scores: most of the order is decided by the ordinal half
        if case.fill == "ties":
            levels = levels[[40, 41]]
        scores = rng.choice(levels, size=total)
        ords = rng.permutation(max(total, 1) * 3)[:total].astype(np.uint64)
        if case.fill == "high":
            ords = np.uint64(2**32 - 2) - ords
        keys = pack_keys(scores, ords)
        at = 0
        for l in range(n):
            lists[l, q, : lens[l]] = np.sort(keys[at : at + lens[l]])[::-1]
            at += lens[l]
    if case.fill == "failed":
        lists[n // 2, 1, :] = FAILED  # the rank's lists of query 1: the failure key in every slot
    return lists


def merged_by_sort(lists: np.ndarray) -> np.ndarray:
    """the reference: the descending uint64 sort of the union of a query's lists, first k (empty slots are 0 and sort last)"""
    n, nq, k = lists.shape
    return np.stack([np.sort(lists[:, q, :].reshape(-1))[::-1][:k] for q in range(nq)])


def merge_branches(n_lists: int, k: int) -> set:
    """what `launch_merge` / `merge_kernel` do with a shape: no more waves than lists (a power of two, at most 16); k <= 64 keeps one key per
    lane and folds four lists per round while four are left for the wave, the rest one by one in the tail loop; k > 64 keeps four keys per
    lane and folds one list per round"""
    waves = 16
    while waves > 1 and waves // 2 >= n_lists:
        waves //= 2
    kpl = 1 if k <= 64 else 4
    g = 4 if kpl == 1 else 1
    quad = tail = 0
    for wave in range(waves):
        m, q, t = wave, 0, 0
        while m + (g - 1) * waves < n_lists:
            q, m = q + 1, m + g * waves
        while m < n_lists:
            t, m = t + 1, m + waves
        quad, tail = max(quad, q), max(tail, t)
    out = {f"kpl{kpl}", f"waves{waves}"}
    if kpl == 1:
        out |= {"tail"} if tail else set()
        out |= {"tail-rounds"} if tail > 1 else set()  # more lists than waves
        out |= {"four-per-round"} if quad else set()
    else:
        assert tail == 0
        out |= {"kpl4-rounds"} if quad > 1 else set()  # more lists than waves
    if n_lists % 2:
        out.add("odd")
    if waves > 1:
        out.add("block-merge")
    return out


# ---- 2. normalise ------------------------------------------------------------------------------------------------------------------------

NORM_VECTOR_WIDTHS = (4, 1532, 1536, 1540, 3072, 4092, 4096, 4100, 4104, 6144)
NORM_SCALAR_WIDTHS = (1537, 3073, 4098)
NORM_GRID_WAVES = 2048 * 4  # launch_normalize_f32: at most 2048 workgroups of four waves, one row per wave and step


@dataclass(frozen=True)
class NormCase:
    name: str
    rows: int
    dim: int
    offset: int = 0  # floats between a 16-byte boundary and the first element (1: a view 4 bytes into a larger buffer)


def _norm_rows(dim: int) -> int:
    return 7 + (dim * 5) % 64  # 7 .. 70: five special rows and at least two plain ones


NORM_CASES = [
    *[NormCase(f"norm-d{d}", _norm_rows(d), d) for d in NORM_VECTOR_WIDTHS + NORM_SCALAR_WIDTHS],
    *[NormCase(f"norm-d{d}-unaligned", _norm_rows(d), d, offset=1) for d in NORM_VECTOR_WIDTHS],
    NormCase("norm-8200x8", 8200, 8),
    NormCase("norm-8195x1540", 8195, 1540),
]

NORM_SPECIAL_ROWS = 5  # row 0 zero, 1 a NaN, 2 a +inf, 3 values of 1e20, 4 a single non-zero element


def norm_branch(case: NormCase) -> set:
    """`launch_normalize_f32` picks the instantiation by the width, the kernel its branch by the width and the two pointers"""
    out = set()
    if case.dim % 4 != 0:
        out.add("scalar")
    elif case.offset % 4 != 0:
        out.add("unaligned-fallback")
    elif case.dim <= 64 * 4 * 6:
        out.add("in-registers-6")
    elif case.dim <= 64 * 4 * 16:
        out.add("in-registers-16")
    else:
        out.add("vector-streamed")
    if case.rows > NORM_GRID_WAVES:
        out.add("grid-stride")
    return out


def norm_input(case: NormCase) -> np.ndarray:
    rng = np.random.default_rng(31_000 + 7 * case.dim + case.rows + case.offset)
    d = case.dim
    x = (rng.standard_normal((case.rows, d)) * 3).astype(np.float32)
    x[0] = 0
    x[1, d // 3] = np.nan
    x[2, d // 2] = np.inf
    x[3, :: max(1, d // 5)] = 1e20  # the squares overflow: the norm is inf and every finite element becomes (+-)0
    x[3, d - 1] = -1e20
    x[4] = 0
    x[4, (2 * d) // 3] = -2.75
    return x


def norm_bound_units(dim: int) -> float:
    """Worst-case relative error of one element of the kernel's y = x / ||x||, in units of 2^-24 (the unit roundoff of float32).
    The sum of squares: every lane chains ceil(dim / 64) fused multiply-adds (one rounding each: the square is exact inside the fma), the
    wave sum is a tree of six additions (four DPP steps and two levels over the four row sums); all terms are non-negative, so each
    rounding is relative to a partial sum that is no larger than the total: (ceil(dim / 64) + 6) units on the sum of squares.  The square
    root halves a relative error and adds one rounding of its own, the division adds one more:
        (ceil(dim / 64) + 6) / 2 + 1 + 1
    (second-order terms are below 1e-5 of that at these widths; the float64 reference itself is good to 2^-50)."""
    return (math.ceil(dim / 64) + 6) / 2 + 2


def norm_check(case: NormCase, x: np.ndarray, y: np.ndarray, oracle: np.ndarray, what: str = "") -> dict:
    """The three assertions on a normalised matrix `y` of `x` (`oracle` = vo.l2_normalize_rows(x)); returns the figures it measured.
      * the special rows equal the oracle's exactly: NaN where it has NaN, the same bits everywhere else;
      * every element of a finite row is within norm_bound_units(dim) * 2^-24 (relative) of the float64 x / ||x||_2;
      * the quotient is an IEEE division: among the float32 values n within that same bound of float32(||x||_2 in float64), at least
        one gives float32(x) / n == y bit for bit over the whole row.  (A reciprocal-multiply differs from every such quotient in some
        element of most rows; a wrong element fails both.)"""
    tag = f"{case.name} {what}".strip()
    assert y.shape == x.shape and y.dtype == np.float32, tag
    s = NORM_SPECIAL_ROWS
    nan = np.isnan(oracle[:s])
    assert np.array_equal(np.isnan(y[:s]), nan), f"{tag}: NaN does not sit where the oracle has NaN (rows 0 .. {s - 1})"
    same = (y[:s].view(np.uint32) == oracle[:s].view(np.uint32)) | nan
    assert same.all(), f"{tag}: special rows differ from the oracle at (row, column) {np.argwhere(~same)[:6].tolist()}"
    xf, yf = x[s:], y[s:]
    x64 = xf.astype(np.float64)
    n64 = np.sqrt((x64 * x64).sum(axis=1))
    ref = x64 / n64[:, None]
    units = norm_bound_units(case.dim)
    err = np.abs(yf.astype(np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ref != 0, err / np.abs(ref), np.where(err == 0, 0.0, np.inf)) * 2.0**24
    worst = float(rel.max())
    assert worst <= units, f"{tag}: an element is {worst:.2f} units of 2^-24 from the float64 quotient, the bound is {units}; at {np.argwhere(rel > units)[:4].tolist()}"
    # the IEEE witness: float32 neighbours of the float64 norm, nearest first, each tried on the rows that have none yet
    n0 = n64.astype(np.float32)
    n0_bits = n0.view(np.uint32).astype(np.int64)
    found = np.zeros(len(xf), dtype=bool)
    steps = np.zeros(len(xf), dtype=np.int64)
    reach = int(math.ceil(units)) + 1  # one float32 step is at least 2^-24 relative
    for j in sorted(range(-reach, reach + 1), key=abs):
        cand = (n0_bits + j).astype(np.uint32).view(np.float32)
        inside = np.abs(cand.astype(np.float64) - n0.astype(np.float64)) <= units * 2.0**-24 * n0.astype(np.float64)
        idx = np.flatnonzero(~found & inside)
        if len(idx) == 0:
            continue
        hit = (xf[idx] / cand[idx, None] == yf[idx]).all(axis=1)
        found[idx[hit]] = True
        steps[idx[hit]] = j
    assert found.all(), (f"{tag}: {int((~found).sum())} of {len(xf)} rows are no IEEE float32 quotient x / n for any n within the bound "
                         f"of the float64 norm; first rows {(np.flatnonzero(~found)[:6] + s).tolist()}")
    return {"worst_units": worst, "bound_units": units, "norm_steps": int(np.abs(steps).max()) if len(steps) else 0}


# ---- 3. convert and the load path --------------------------------------------------------------------------------------------------------

CONV_GRID_THREADS = 2048 * 256  # launch_f32_to_f16: at most 2048 workgroups of 256 lanes, eight elements per lane and step
CONV_BIG = CONV_GRID_THREADS * 8 + 8 * 300 + 5

CONV_SPECIALS = np.array(
    [0.0, -0.0, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, np.inf, -np.inf,  # 65519.99 stays 65504, 65520 is the first to become inf
     2.0**-24, 2.0**-25, 1.5 * 2.0**-25, 6.0e-5, -(2.0**-24), -(2.0**-25), 3.0 * 2.0**-25, np.nan]  # the half subnormals, a tie at zero
    + [1 + (2 * j + 1) * 2.0**-11 for j in range(8)],  # ties between two halves: to even
    dtype=np.float32)


@dataclass(frozen=True)
class ConvCase:
    name: str
    count: int
    offset: int = 0  # floats between a 16-byte boundary and the first input element


CONV_CASES = [
    ConvCase("conv-big", CONV_BIG),
    ConvCase("conv-big-unaligned", CONV_BIG, offset=1),
    *[ConvCase(f"conv-n{n}", n) for n in (1, 7, 8, 9)],
    *[ConvCase(f"conv-n{n}-unaligned", n, offset=1) for n in (1, 9)],
]


def conv_branches(case: ConvCase) -> set:
    blocks = min(max((case.count // 8 + 255) // 256, 1), 2048)
    threads = blocks * 256
    if case.offset % 4 != 0:
        return {"unaligned"} | ({"unaligned-grid-stride"} if case.count > threads else set())
    out = set()
    if case.count // 8 > 0:
        out.add("vector")
    if case.count % 8:
        out.add("tail")
    if case.count // 8 > threads:
        out.add("grid-stride")
    return out


def conv_input(case: ConvCase) -> np.ndarray:
    """Gaussians with the special values at the head, behind the first pass of the grid (elements only the grid-stride loop reaches) and
    in the last elements (the scalar tail); the short counts take a window of the special values each"""
    rng = np.random.default_rng(41_000 + case.count)
    n, s = case.count, len(CONV_SPECIALS)
    x = rng.standard_normal(n).astype(np.float32)
    if n < 3 * s:
        x[:] = np.roll(CONV_SPECIALS, -{1: 0, 7: 1, 8: 8, 9: 16}.get(n, 0))[:n]  # the four short counts carry every special value between them
        return x
    x[:s] = CONV_SPECIALS
    x[n - s:] = CONV_SPECIALS[::-1]
    edge = CONV_GRID_THREADS * 8
    if n > edge + s:
        x[edge - 3 : edge - 3 + s] = CONV_SPECIALS
    return x


def conv_check(x: np.ndarray, y: np.ndarray, what: str):
    """bit for bit `x.astype(np.float16)`; where the input is NaN only that the output is NaN"""
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert y.dtype == np.float16 and y.shape == x.shape, what
    nan = np.isnan(x)
    assert np.isnan(y[nan]).all(), f"{what}: a NaN came out as a number"
    diff = (y.view(np.uint16) != want.view(np.uint16)) & ~nan
    assert not diff.any(), (f"{what}: {int(diff.sum())} of {x.size} elements differ from round-to-nearest-even; first at {np.flatnonzero(diff.reshape(-1))[:6].tolist()}: "
                            f"{x.reshape(-1)[np.flatnonzero(diff.reshape(-1))[:6]].tolist()}")


UPLOAD_SLOT_BYTES = 16 << 20  # tavb_upload_rows: rows go through pinned staging slots of 16 MiB


@dataclass(frozen=True)
class UploadCase:
    name: str
    rows: int
    dim: int
    parts: tuple  # rows per `upload_rows` call, in order (appends)
    dtype: str  # "fp16" / "fp32"
    seed: int


UPLOAD_CASES = [UploadCase(f"upload-{rows}x{dim}-{dt}", rows, dim, parts, dt, 51_000 + dim)
                for rows, dim, parts in ((2500, 4099, (2500,)), (300, 33, (1, 10, 289))) for dt in ("fp16", "fp32")]


def upload_chunks(case: UploadCase) -> list:
    """[(first row, rows, destination byte offset mod 16)] of every staging chunk of every call: the destination buffer itself starts on a
    16-byte boundary (the allocator's), a chunk starts `first row * dim * element size` bytes into it"""
    elem = 2 if case.dtype == "fp16" else 4
    per = max(1, UPLOAD_SLOT_BYTES // (case.dim * 4))
    out, start = [], 0
    for n in case.parts:
        done = 0
        while done < n:
            m = min(per, n - done)
            out.append((start + done, m, ((start + done) * case.dim * elem) % 16))
            done += m
        start += n
    return out


def upload_input(case: UploadCase):
    return make_corpus(case.rows, case.dim, case.seed)


# ---- 4. remap ----------------------------------------------------------------------------------------------------------------------------

REMAP_GRID_THREADS = 1024 * 256
OUT_OF_RANGE = np.uint64(0xFFFFFFFE)  # the ordinal a position behind the map becomes


@dataclass(frozen=True)
class RemapCase:
    name: str
    count: int
    map_len: int


REMAP_CASES = [RemapCase("remap-300000-map1000", 300_000, 1000), RemapCase("remap-5000-map1", 5000, 1), RemapCase("remap-1-map1000", 1, 1000)]


def remap_input(case: RemapCase):
    """(keys uint64 [count], map int32 [map_len]): key i carries a random position into the map; one key in seven (i % 7 == 3) is 0, one in
    eleven (i % 11 == 5) carries a position >= map_len; key 0 carries the LAST position of the map, key 2 the first one behind it"""
    rng = np.random.default_rng(61_000 + case.count + case.map_len)
    n, ml = case.count, case.map_len
    i = np.arange(n)
    pos = rng.integers(0, ml, size=n).astype(np.uint64)
    behind = np.array([ml, ml + 1, ml + 4096, 2**31, 2**32 - 2], dtype=np.uint64)
    far = i % 11 == 5
    pos[far] = behind[rng.integers(0, len(behind), size=int(far.sum()))]
    pos[0] = ml - 1
    if n > 2:
        pos[2] = ml
    scores = rng.uniform(0.01, 1.0, size=n).astype(np.float32)
    keys = pack_keys(scores, pos)
    keys[i % 7 == 3] = 0
    m = rng.integers(0, 2**31 - 1, size=ml).astype(np.int32)
    m[-1] = 2**31 - 2
    if ml > 1:
        m[0] = 0
    return keys, m


def remap_reference(keys: np.ndarray, m: np.ndarray) -> np.ndarray:
    pos = U32 - (keys & U32)
    to = np.where(pos < np.uint64(len(m)), m.astype(np.uint32).astype(np.uint64)[np.minimum(pos, np.uint64(len(m) - 1)).astype(np.int64)], OUT_OF_RANGE)
    return np.where(keys == 0, np.uint64(0), (keys & HI) | (U32 - to))


# ---- 5. re-rank --------------------------------------------------------------------------------------------------------------------------

RERANK_ROWS, RERANK_DIM, RERANK_SEED = 2000, 64, 71_000
RERANK_MIN_GAP = 2e-6  # between neighbouring float64 scores of the hits: the order of the float32 lookups is then the oracle's
ACCEPT_LONG = 300_000  # more than the bitmap kernel's grid of 1024 x 256 lanes


@dataclass(frozen=True)
class RerankCase:
    name: str
    form: str  # "embedding" (lookup_messages_by_embedding: the whole corpus, an optional accept collection) / "subset" (lookup_messages_in_subset)
    rows_map: str  # "one" (every row in message 0), "own" (row r in message r), "none" (all -1), "blocks" (7 rows per message)
    max_matches: int
    accept: str = "none"  # "none", "even" (the even messages), "long-head" (300 000 integers, only the first 150 below the message count),
    #                       "long-tail" (the same with those 150 at the END: behind the first pass of the bitmap kernel's grid)


_RERANK_MAPS = (("one", 256), ("own", 256), ("own", 255), ("none", 256), ("blocks", 1), ("blocks", 37), ("blocks", 256))
RERANK_CASES = [
    *[RerankCase(f"rerank-{m}-mm{mm}-{a}", "embedding", m, mm, a) for m, mm in _RERANK_MAPS for a in ("none", "even", "long-head", "long-tail")],
    *[RerankCase(f"rerank-subset-{m}-mm{mm}", "subset", m, mm) for m, mm in _RERANK_MAPS],
]


def rerank_corpus():
    return make_corpus(RERANK_ROWS, RERANK_DIM, RERANK_SEED)


def rerank_map(kind: str) -> np.ndarray:
    r = np.arange(RERANK_ROWS, dtype=np.int64)
    return {"one": r * 0, "own": r, "none": r * 0 - 1, "blocks": r // 7}[kind]


def rerank_accept(kind: str, n_messages: int):
    if kind == "none":
        return None
    if kind == "even":
        return list(range(0, n_messages, 2))
    live = (np.arange(150, dtype=np.int64) * 13) % max(n_messages, 1)  # (150 ordinals below the message count, where there is one)
    dead = np.random.default_rng(72_000).integers(max(n_messages, 1), 2**31 - 1, size=ACCEPT_LONG - 150)
    return np.concatenate([live, dead] if kind == "long-head" else [dead, live])


def rerank_subset() -> list:
    # (a seed under which the hits of the subset keep RERANK_MIN_GAP as well: the CPU twin asserts it)
    return np.random.default_rng(73_004).choice(RERANK_ROWS, size=1200, replace=False).tolist()
