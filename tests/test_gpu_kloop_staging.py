"""GPU suite: the staging state of the wide tile's K loop (tavb_mfma_wide.hip) where a value carried from step to step can go wrong.

The stager keeps the corpus descriptor of the tile being staged, the scalar offsets of the slab and its LDS slot as running values that
move on behind the last piece of a slab; the staging runs one to two slabs ahead of the MFMAs, across tile boundaries.  The shapes here are
the smallest at which that can break: D = 64 is ONE K step per tile (the slab wraps, and the descriptor moves on, in every step, and the
run-ahead always crosses a tile boundary), D = 128 / 192 two and three steps (an odd count starts the next tile in the other LDS slot), D = 1536
the benchmark's 24; row counts give a last piece of fewer than 8 rows, exactly one tile, one row over, a partial tile behind a full one, and
three and more tiles per workgroup, where the reloads past the last tile of a row range run.

Every case asserts through `last_tier` / `last_mfma_shape` that the wide tile ran, runs k = 32 and k = 256 (every block class of a tile returns
a row) at threshold 0 and at one that leaves a handful of rows, compares the keys of mfma_shape = 16 and 32 bit for bit in one process, and
checks sampled queries against the float64-refereed oracle as the neighbouring suites do.
"""

from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

DIMS = (64, 128, 192, 1536)
ROWS = (7, 319, 320, 321, 647, 8 * 320 * 3 + 5)
FORCE_WIDE = (("direct_group_max_nq", 0), ("mfma_min_batch", 32), ("mfma_min_batch_f32", 32))
BASE = (1 << 31) + 12345


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=None)
def _queries(dim: int):
    return make_queries(1024, dim, 7300 + dim)


@functools.lru_cache(maxsize=8)
def _gauss(rows: int, dim: int, dtype: str):
    """-> (the values the kernels multiply as float32, what is stored)"""
    v, _ = make_corpus(rows, dim, 7100 + dim + rows)
    if dtype == "fp16":
        v16 = v.astype(np.float16)
        return v16.astype(np.float32), v16
    return v, v


def _engine(store: np.ndarray, opts, base: int = 0):
    dev = _torch().from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*FORCE_WIDE, *opts):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev, ordinal_base=base)
    return eng, dev


def _lookup(eng, dq, k: int, thr: float, shape: int, want_shape: int, what: str):
    torch = _torch()
    eng.set_option("mfma_shape", shape)
    out = torch.zeros((dq.shape[0], k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_device(dq, k, thr, out_keys=out)
    eng.synchronize()
    state = {g: eng.get_option(g) for g in ("last_tier", "last_mfma_shape")}
    assert state == {"last_tier": 4, "last_mfma_shape": want_shape}, f"{what}: the wide tile did not run as asked: {state}"
    return out.cpu().numpy().copy()


def _check(eng, v, qs, base: int, shapes, what: str, sample=None):
    """k = 32 and 256 x threshold 0 and a handful-of-rows threshold: the shapes' keys identical, sampled queries against the oracle.
    shapes: ((mfma_shape, the shape last_mfma_shape must report), ...).  -> last_flagged of the threshold-0, k = 32 run"""
    torch = _torch()
    nq = qs.shape[0]
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    rows = v.shape[0]
    handful = float(np.sort(vo.scores_full(v, qs[0]))[::-1][min(3, rows - 1)])
    flagged = None
    for k in (32, 256):
        for thr in (0.0, handful):
            t32 = float(_native.f32_threshold(thr))
            keys = None
            for shape, want in shapes:
                got = _lookup(eng, dq, k, t32, shape, want, f"{what} k={k} thr={thr} shape={shape}")
                if flagged is None:
                    flagged = eng.get_option("last_flagged")
                if keys is None:
                    keys = got
                else:
                    diff = got != keys
                    assert not diff.any(), f"{what} k={k} thr={thr}: {int(diff.sum())} of {got.size} keys differ between the MFMA shapes, first at {np.argwhere(diff)[:4].tolist()}"
            ords, scs, cnts = _native.decode_keys(keys)
            if thr == 0.0:
                assert (cnts == min(k, rows)).all(), f"{what} k={k}: counts {np.unique(cnts).tolist()}"
            else:
                assert cnts[0] >= 1  # (query 0's own threshold; the oracle decides each count)
            # Both shapes share the stager, so only the oracle can see a wrong offset on one query piece.  A piece is 8 consecutive queries: up
            # to 2003 rows every 7th query is refereed at k = 32 (every piece of every wave of every query tile), otherwise the corners.
            dense = set(range(0, nq, 7)) if rows <= 2003 and k == 32 else set()
            for qi in sorted(sample or ({0, 1, nq // 2, nq - 1} | dense)):
                m = int(cnts[qi])
                vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m] - base, scs[qi, :m], k, thr, referee=vo.f64_referee(v, qs[qi]))
    return flagged


BOTH = ((16, 16), (32, 32))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("dim", DIMS)
def test_row_tails_and_tile_wraps(dim, rows):
    """256 and 1024 queries on the 256-query tile.  The longest corpus runs on 8 row ranges: at least three tiles per workgroup."""
    v, store = _gauss(rows, dim, "fp16")
    eng, dev = _engine(store, (("mfma_tile", 256), ("mfma_splits", 8 if rows > 647 else 0)))
    try:
        for nq in (256, 1024):
            _check(eng, v, _queries(dim)[:nq], 0, BOTH, f"D={dim} rows={rows} nq={nq}")
    finally:
        eng.close()


@pytest.mark.parametrize("dim", DIMS)
def test_ragged_split_with_ordinal_base_above_2_31(dim):
    """2003 rows on 3 row ranges of 960 rows (the last one short and ending inside a tile), ordinals from 2^31 + 12345."""
    v, store = _gauss(2003, dim, "fp16")
    eng, dev = _engine(store, (("mfma_tile", 256), ("mfma_splits", 3)), base=BASE)
    try:
        _check(eng, v, _queries(dim)[:256], BASE, BOTH, f"D={dim} rows=2003 base")
    finally:
        eng.close()


@pytest.mark.parametrize("rows", (321, 2000))
@pytest.mark.parametrize("dim", DIMS)
def test_128_query_tile(dim, rows):
    """100 queries on the 128-query tile: three corpus slots, the query slab staged first, a counted wait (always 32x32x16)."""
    v, store = _gauss(rows, dim, "fp16")
    eng, dev = _engine(store, (("mfma_tile", 128),))
    try:
        _check(eng, v, _queries(dim)[:100], 0, ((16, 32),), f"D={dim} rows={rows} tile=128")
    finally:
        eng.close()


def test_split_plane_form_on_duplicates():
    """2000 rows of which 1500 are near-duplicates of one centre, 300 queries near it, a 256-key band: the queries are flagged and re-run on the
    SPLIT form, whose K loop walks the corpus columns twice and jumps to the queries' low plane half way."""
    dim, rows, cluster = 128, 2000, 1500
    rng = np.random.default_rng(7400)
    centre = rng.standard_normal(dim).astype(np.float32)
    centre /= np.linalg.norm(centre)
    v, _ = make_corpus(rows, dim, 7401)
    member = rng.permutation(rows)[:cluster]
    near = centre[None, :] + 0.002 * rng.standard_normal((cluster, dim)).astype(np.float32) / np.sqrt(dim)
    v[member] = near / np.linalg.norm(near, axis=1, keepdims=True)
    # (queries a little way off the centre, scores near 0.9994: at the centre itself float32 and float64 scores are both clipped to exactly 1 and
    #  the oracle's near-tie width, which it measures from their difference, is zero among rows that tie)
    qs = centre[None, :] + 0.05 * rng.standard_normal((300, dim)).astype(np.float32) / np.sqrt(dim)
    qs = np.ascontiguousarray(qs / np.linalg.norm(qs, axis=1, keepdims=True), dtype=np.float32)
    v16 = v.astype(np.float16)
    eng, dev = _engine(v16, (("mfma_tile", 256), ("band_max", 256)))
    try:
        flagged = _check(eng, v16.astype(np.float32), qs, 0, BOTH, "duplicates D=128", sample=set(range(0, 300, 7)))
        assert flagged > 0, f"last_flagged {flagged}: the split-plane form did not run"
    finally:
        eng.close()


def test_fp32_rows_take_the_shadow():
    """256 queries over 2000 fp32 rows at D = 128: the filter stages the fp16 shadow of the rows."""
    v, store = _gauss(2000, 128, "fp32")
    eng, dev = _engine(store, (("mfma_tile", 256),))
    try:
        _check(eng, v, _queries(128)[:256], 0, BOTH, "fp32 D=128 rows=2000")
        assert eng.get_option("last_shadow") == 1
    finally:
        eng.close()
