"""GPU suite: the 256-query filter tile in both MFMA shapes at every width, row tail and query tail (the table is tests/wide256_cases.py).

tests/test_gpu_mfma_shape.py compares the two shapes at D = 1536 on corpora of 60 000 rows and more with k up to 256: there most (row position,
query position) classes of a tile are never hit by a returned row, the K loop has an even number of steps, and a row range ends wherever the
corpus happens to.  Here the corpora are a few hundred rows and k is 256, so every query returns a large share of the corpus and every block class
of the tile is exercised (tests/test_wide256_cases_host.py asserts that of the inputs); widths give K loops of 1, 2, 3, 5, 15, 24, 48 and 64 steps
(an odd count starts the next tile in the other LDS slot); row counts end a range one below, on and one above every granularity of the epilogue.

Every case forces tier 4 and the 256-query tile (`direct_group_max_nq = 0`, `mfma_tile = 256`, `mfma_min_batch` low) and runs the lookup three
times: mfma_shape = 16, mfma_shape = 32, and the 128-query tile (always 32x32x16) -- `last_tier`, `last_mfma_shape`, `last_shadow` and
`last_flagged` say what ran.  The three key arrays must be identical in all nq x k slots; EVERY query is checked against the float64-refereed
oracle with the project's tolerances; for a handful of queries the batch entry equals the single lookup bit for bit (the rescored tiles carry
the streaming kernels' float32 scores).

What each kind of case can see: a corpus with fewer rows than k returns every row at threshold 0, so the row tails below 256 rows check the row
bound of the epilogue (no row lost, none invented) and are blind to a permutation of rows inside a tile; a wrong accumulator-to-row map is
caught by the cases with more rows than k.  With `r_off = 16 * m + (j ^ 1)` in the 16x16x32 epilogue, 81 of the 113 cases fail (every width,
compaction, query-tail, k, ladder and base case and every row tail of 319 rows and more, first on the keys differing from the 32x32x16 run);
the 32 row tails of 1 to 241 rows pass.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import wide256_cases as wc
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

# (mfma_shape, mfma_tile) -> the shape the filter must report
RUNS = ((16, 256, 16), (32, 256, 32), (16, 128, 32))
# Fills the output rows behind the batch.  The filter pads a batch to whole 256-query tiles and gives each padding query a threshold of +inf, so it
# admits nothing; select and rescore are launched for the live queries only, so what a padding query admitted into the candidate buffer has no
# getter or counter of its own.  What IS observable, and asserted: no output row behind the last live query is written, every slot of a live
# query is, and the live queries next to the padding (the last three, the first of the last 16-query fragment and of the last tile) equal their
# single lookups bit for bit -- a padding query that spilt into a neighbour's count or candidates would break that.
SENTINEL = -0x0123456789ABCDEF


def _torch():
    import torch

    return torch


def _engine(case: wc.Case, store: np.ndarray):
    torch = _torch()
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (("direct_group_max_nq", 0), ("mfma_min_batch", 32), ("mfma_min_batch_f32", 32), *case.opts):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev, ordinal_base=case.base)
    return eng, dev


def _assert_route(eng, case: wc.Case, want_shape: int, what: str):
    state = {g: eng.get_option(g) for g in ("last_tier", "last_mfma_shape", "last_shadow", "last_flagged")}
    assert state["last_tier"] == 4, f"{case.name} {what}: {state}"
    assert state["last_mfma_shape"] == want_shape, f"{case.name} {what}: {state}"
    assert state["last_shadow"] == int(case.padded), f"{case.name} {what}: {state}"
    assert state["last_flagged"] == 0, f"{case.name} {what}: {state}"


def _device_runs(eng, case: wc.Case, dq, thr: float):
    """the three runs under every mfma_splits of the case -> {(splits, shape, tile): keys [nq, k]}; rows behind the batch stay untouched"""
    torch = _torch()
    nq_pad = (case.nq + wc.TILE_QUERIES - 1) // wc.TILE_QUERIES * wc.TILE_QUERIES
    got = {}
    for splits in case.splits:
        eng.set_option("mfma_splits", splits)
        for shape, tile, want_shape in RUNS:
            eng.set_option("mfma_shape", shape)
            eng.set_option("mfma_tile", tile)
            out = torch.full((nq_pad + 1, case.k), SENTINEL, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            if case.group == "ladder":
                eng.profile_reset()
            eng.search_device(dq, case.k, thr, out_keys=out)
            eng.synchronize()
            what = f"splits {splits} shape {shape} tile {tile}"
            _assert_route(eng, case, want_shape, what)
            if case.group == "ladder":  # the phases the options ask for ran: one launch each
                phases = len(wc.case_ladder_bounds(case)) - 1
                assert phases >= 3
                assert eng.profile_read(_native.KERNEL_MFMA_SAMPLE)[1] == phases - 1 and eng.profile_read(_native.KERNEL_MFMA)[1] == 1, what
            host = out.cpu().numpy()
            assert (host[case.nq:] == SENTINEL).all(), f"{case.name} {what}: keys written behind the last live query"
            assert not (host[: case.nq] == SENTINEL).any(), f"{case.name} {what}: slots of a live query left unwritten"
            got[(splits, shape, tile)] = host[: case.nq].copy()
    return got


def _assert_identical(case: wc.Case, got: dict):
    first_name, first = next(iter(got.items()))
    for name, keys in got.items():
        diff = keys != first
        assert not diff.any(), (f"{case.name}: (mfma_splits, mfma_shape, mfma_tile) = {name} and {first_name} differ in {int(diff.sum())} of {keys.size} keys; "
                                f"first at (query, slot) {np.argwhere(diff)[:4].tolist()}")
    return first


def _check_oracle(case: wc.Case, v, qs, ords, scs, cnts, thrs):
    """every query against the float64-refereed oracle"""
    for qi in range(case.nq):
        m = int(cnts[qi])
        try:
            vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], case.k, float(thrs[qi]), referee=vo.f64_referee(v, qs[qi]))
        except AssertionError as e:
            want = set(wc.oracle_topk_rows(v, qs[qi: qi + 1], case.k)[0].tolist())
            missing = sorted(want - set(ords[qi, :m].tolist()))
            raise AssertionError(f"{case.name}: query {qi} (lane {qi % 16} of 16-query fragment {qi // 16}): {e}; of the float64 top {case.k} missing rows "
                                 f"{missing[:12]} (row mod 320: {[r % 320 for r in missing[:12]]})") from e


def _singles(case: wc.Case):
    nq = case.nq
    near_padding = {nq - 1, nq - 2, nq - 3, (nq - 1) // 16 * 16, (nq - 1) // 256 * 256}
    return sorted(q for q in ({0, 1, 17, nq // 2} | near_padding | set(wc.planted(case))) if 0 <= q < nq)[:24]


def _check_singles(case: wc.Case, eng, qs, ords, scs, cnts, thrs):
    """the batch entry of a query is its single lookup, bit for bit (`ords` are rows: the caller took the ordinal base off)"""
    for qi in _singles(case):
        so, ss = eng.search(qs[qi], case.k, np.float32(thrs[qi]))
        m = int(cnts[qi])
        assert ords[qi, :m].tolist() == (np.asarray(so, dtype=np.int64) - case.base).tolist() and scs[qi, :m].tolist() == ss.tolist(), (case.name, qi)


UNIFORM = [c for c in wc.CASES if c.thr != "mixed"]
MIXED = [c for c in wc.CASES if c.thr == "mixed"]


@pytest.mark.parametrize("case", UNIFORM, ids=[c.name for c in UNIFORM])
def test_wide256_case(case):
    """One case of the table through `search_device`; every run asserts the tile and the MFMA shape that actually ran (`_assert_route`)."""
    torch = _torch()
    v, store, qs = wc.case_inputs(case)
    eng, dev = _engine(case, store)
    if case.group == "ladder":
        eng.profile_enable(True)
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    thr = 0.0
    if case.thr == "fifth":
        thr = float(np.sort(vo.scores_full(v, qs[0]))[::-1][4])
    t32 = float(_native.f32_threshold(thr))
    keys = _assert_identical(case, _device_runs(eng, case, dq, t32))
    ords, scs, cnts = _native.decode_keys(keys)
    ords = ords - case.base
    thrs = np.full(case.nq, t32, dtype=np.float32)
    if case.thr == "zero":  # every row survives threshold 0: a corpus shorter than k comes back whole
        assert (cnts == min(case.k, case.rows)).all(), f"{case.name}: counts {np.unique(cnts).tolist()}"
        if case.rows <= case.k:
            assert (np.sort(ords[:, : case.rows], axis=1) == np.arange(case.rows)[None, :]).all()
    else:
        assert cnts[0] >= 1 and cnts.min() < case.k  # (sparse: the oracle decides each count)
    _check_oracle(case, v, qs, ords, scs, cnts, thrs)
    for qi, row in wc.planted(case).items():
        assert ords[qi, 0] == row, f"{case.name}: the copy of query {qi} in row {row} (row mod 320 = {row % 320}) does not rank first: {ords[qi, :3].tolist()}"
    if case.base:  # the base-0 keys with every ordinal shifted, scores bit for bit
        eng0, dev0 = _engine(wc.Case(case.name, case.group, case.dtype, case.rows, case.dim, nq=case.nq, k=case.k, seed=case.seed), store)
        eng0.set_option("mfma_tile", 256)
        base0 = eng0.search_device(dq, case.k, t32)
        eng0.synchronize()
        assert eng0.get_option("last_tier") == 4 and eng0.get_option("last_mfma_shape") == 16
        np.testing.assert_array_equal(keys, wc.shift_keys(base0.cpu().numpy(), case.base), err_msg=case.name)
        eng0.close()
    _check_singles(case, eng, qs, ords, scs, cnts, thrs)
    eng.close()


@pytest.mark.parametrize("case", MIXED, ids=[c.name for c in MIXED])
def test_wide256_mixed_thresholds(case):
    """One threshold per query through `search_batch` (a NaN and a value above 1 among them, as test (f) of tests/test_gpu_routes.py): the same
    three runs, identical answers, every query against the oracle and against its single lookup with that threshold."""
    v, store, qs = wc.case_inputs(case)
    eng, dev = _engine(case, store)
    s0 = np.sort(vo.scores_full(v, qs[0]))[::-1]
    lo, hi = 0.0, float(s0[4])
    pattern = [lo, hi, float("nan"), 1.5, lo + (hi - lo) / 2]
    t = np.array([_native.f32_threshold(pattern[i % len(pattern)]) for i in range(case.nq)], dtype=np.float32)
    got = {}
    for shape, tile, want_shape in RUNS:
        eng.set_option("mfma_shape", shape)
        eng.set_option("mfma_tile", tile)
        ords, scs, cnts = eng.search_batch(qs, case.k, t)
        state = {g: eng.get_option(g) for g in ("last_tier", "last_mfma_shape", "last_shadow", "last_flagged")}
        assert state == {"last_tier": 4, "last_mfma_shape": want_shape, "last_shadow": 0, "last_flagged": 0}, (case.name, shape, tile, state)
        for qi in range(case.nq):  # (slots past a query's count are not part of the answer)
            ords[qi, cnts[qi]:] = -1
            scs[qi, cnts[qi]:] = 0
        got[(shape, tile)] = (ords, scs, cnts)
    ords, scs, cnts = got[(16, 256)]
    for name, (o, s, c) in got.items():
        assert np.array_equal(c, cnts) and np.array_equal(o, ords) and np.array_equal(s.view(np.uint32), scs.view(np.uint32)), (case.name, name)
    dead = np.isnan(t) | (t > 1)
    assert dead.any() and (cnts[dead] == 0).all()
    assert (cnts[t == 0] == case.k).all() and cnts[1] < case.k
    live = np.flatnonzero(~dead)
    for qi in live:
        m = int(cnts[qi])
        vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], case.k, float(t[qi]), referee=vo.f64_referee(v, qs[qi]))
    for qi in live[:10].tolist() + live[-5:].tolist():
        so, ss = eng.search(qs[qi], case.k, t[qi])
        m = int(cnts[qi])
        assert ords[qi, :m].tolist() == so.tolist() and scs[qi, :m].tolist() == ss.tolist(), (case.name, qi)
    eng.close()
