"""GPU suite: the 32/64-query tile (`skinny_scan_kernel`) in all 14 instantiations, at every K-loop length around its rings, every row tail,
forced row ranges and every query tail (the table is tests/skinny_cases.py; tests/test_skinny_cases_host.py asserts the table's own claims).

The scores of this tile leave the engine as the tile computed them -- the routes tile32-* / tile64-* of tests/test_gpu_routes.py rescore
nothing -- so a wrong fragment map, swizzle or wait count here is a wrong answer, not a lost candidate.  The other suites run the tile at
D = 1536, 384 and 64 (whole-line widths, the ring variant, two K steps at the least) on row counts the library cut into ranges itself.  Here
the corpora are a few hundred rows and k is 64, the tile's maximum, so every query returns a large share of the corpus and every block class
of a tile holds a returned pair; widths give K loops of 1, 2, 3, 4, 5, 24, 48 and 49 steps of 128 and of 64 bytes; row counts end a range one
below, on and one above every granularity of the epilogue; `mfma_splits` forces one workgroup over several tiles (compaction between tiles at
threshold 0), empty row ranges and a range count that is no multiple of 8.  A run under a forced `mfma_splits` must be ONE launch (the profile
counters say so): the compaction cases ask for one phase (`mfma_sample_rows = -1`), since by default a single range of 1024 rows and more is
scanned as a seeding tile and the rest behind its thresholds, which never fills a buffer.

Every case forces tier 5 (`skinny_cases.ROUTE_OPTS`) and runs the lookup several ways (`skinny_cases.runs`): its first 32 queries (32-query
tile), all 64 (64-query tile), on whole-line widths the 32 again under `mfma_sched` 8 (deep ring), 6 (half tiles of 128 rows), 5 (register
staging) and 9 (64-byte steps), all under every `mfma_splits` of the case.  After every call `last_tier`, `last_shadow` and
`last_skinny_kernel` say what ran.  All runs must give identical keys in all nq x k slots, bit for bit: every instantiation issues the same
MFMA sequence over k for a given (row, query), and the selection is exact.  EVERY query is then checked against the float64-refereed oracle at
the project's tolerances, on the values the kernel multiplies (the fp16-rounded rows of an fp16 corpus, the unrounded queries).

What each kind of case can see.  The scores travel with the rows, so even a corpus of at most k rows, which comes back whole at threshold 0,
shows a permutation of rows inside a block as scores on the wrong rows; only a corpus of ONE row is blind to the row map (the rows of a tile
behind the end of the corpus are reloads of the last row: every accumulator row holds row 0's scores).  The planted copies (the last row of
the corpus and of every complete 32-row block of the last tile must rank first) name the block a wrong map hits.

Mutations of the kernel, each built into a scratch copy of the library and run once over the 243 cases of this file:
  * `r_off = (j ^ 1) + 8 * g` in the epilogue's row map: 239 cases fail, first on the oracle's score check; the four row tails of one row pass.
  * `SH = 1` for `STEP == 64` (the swizzle term of the 64-byte steps): 0 cases fail, and none can: the term is applied to the source address
    of the staging loads and to the fragment reads alike, so the mutant moves rows to other bank slots and reads them back from there -- the
    same values, with LDS bank conflicts.  It is a mutant of speed, not of the answer.
  * the same term on the fragment reads ONLY (`frag_row >> 1` for `STEP == 64`, the staging side left alone): all 243 cases fail -- the
    half-line widths on their own kernels, the whole-line widths on their run under `mfma_sched = 9`.
"""

from __future__ import annotations

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import skinny_cases as sc
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

# Fills the output rows behind the batch and every slot before the call.  The tile pads a batch to whole 32- or 64-query tiles and gives each
# padding query a threshold of +inf; no output row behind the last live query may be written, and every slot of a live query must be.
SENTINEL = -0x0123456789ABCDEF
GETTERS = ("last_tier", "last_shadow", "last_skinny_kernel")


def _torch():
    import torch

    return torch


def _engine(case: sc.Case, store: np.ndarray, base: int | None = None):
    torch = _torch()
    dev = torch.from_numpy(store).cuda()
    eng = _native.Engine(0)
    for name, val in (*sc.ROUTE_OPTS, *case.opts):
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev, ordinal_base=case.base if base is None else base)
    return eng, dev


def _assert_route(eng, case: sc.Case, run: sc.Run):
    state = {g: eng.get_option(g) for g in GETTERS}
    assert state == {"last_tier": 5, "last_shadow": 0, "last_skinny_kernel": run.kernel}, f"{case.name} {run.what}: want kernel {run.kernel}, got {state}"


def _device_runs(eng, case: sc.Case, dq, thr: float) -> dict:
    """every run of the case -> {run: keys [run.nq, k]}; rows behind the batch stay untouched"""
    torch = _torch()
    got = {}
    for run in sc.runs(case):
        eng.set_option("mfma_splits", run.splits)
        eng.set_option("mfma_sched", run.sched)
        out = torch.full(((run.nq + 63) // 64 * 64 + 1, case.k), SENTINEL, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        counted = case.group == "ladder" or run.splits > 0
        if counted:
            eng.profile_reset()
        eng.search_device(dq[: run.nq], case.k, thr, out_keys=out)
        eng.synchronize()
        _assert_route(eng, case, run)
        if counted:  # the phases asked for ran, one launch each: three in the ladder group, ONE under a forced mfma_splits (no seeding phase)
            phases = len(sc.case_ladder_bounds(case) if case.group == "ladder" else sc.case_phase_bounds(case, run.splits)) - 1
            launches = (eng.profile_read(_native.KERNEL_MFMA_SAMPLE)[1], eng.profile_read(_native.KERNEL_SKINNY)[1])
            assert phases == (3 if case.group == "ladder" else 1) and launches == (phases - 1, 1), f"{case.name} {run.what}: {launches} launches for {phases} phases"
        host = out.cpu().numpy()
        assert (host[run.nq:] == SENTINEL).all(), f"{case.name} {run.what}: keys written behind the last live query"
        assert not (host[: run.nq] == SENTINEL).any(), f"{case.name} {run.what}: slots of a live query left unwritten"
        got[run] = host[: run.nq].copy()
    eng.set_option("mfma_splits", 0)
    eng.set_option("mfma_sched", 0)
    return got


def _assert_identical(case: sc.Case, got: dict) -> np.ndarray:
    """-> the keys of the whole batch; every run equals them in its own queries"""
    full_run, full = next((r, k) for r, k in got.items() if r.nq == case.nq and r.sched == 0)
    for run, keys in got.items():
        diff = keys != full[: run.nq]
        if diff.any():
            where = np.argwhere(diff)
            o_a, _, _ = _native.decode_keys(keys)
            o_b, _, _ = _native.decode_keys(full[: run.nq])
            q0 = int(where[0][0])
            only = sorted(set((o_a[q0] - case.base).tolist()) ^ set((o_b[q0] - case.base).tolist()))
            raise AssertionError(
                f"{case.name}: run ({run.what}, kernel {run.kernel}) and run ({full_run.what}, kernel {full_run.kernel}) differ in {int(diff.sum())} of "
                f"{keys.size} keys; first at (query, slot) {where[:4].tolist()}; query {q0} = lane {q0 % 32} of 32-query block {q0 // 32}: rows in one "
                f"answer only {only[:12]} (row mod 256: {[r % 256 for r in only[:12]]})")
    return full


def _check_oracle(case: sc.Case, v, qs, ords, scs, cnts, thrs):
    """every query against the float64-refereed oracle"""
    for qi in range(case.nq):
        m = int(cnts[qi])
        try:
            vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], case.k, float(thrs[qi]), referee=vo.f64_referee(v, qs[qi]))
        except AssertionError as e:
            want = set(sc.oracle_topk_rows(v, qs[qi: qi + 1], case.k)[0].tolist())
            missing = sorted(want - set(ords[qi, :m].tolist()))
            raise AssertionError(f"{case.name}: query {qi} (lane {qi % 32} of 32-query block {qi // 32}): {e}; of the float64 top {case.k} missing rows "
                                 f"{missing[:12]} (row mod 256: {[r % 256 for r in missing[:12]]})") from e


def _check_planted(case: sc.Case, ords):
    for qi, row in sc.planted(case).items():
        assert ords[qi, 0] == row, (f"{case.name}: the copy of query {qi} (lane {qi % 32} of block {qi // 32}) in row {row} (row mod 256 = {row % 256}) does "
                                    f"not rank first: {ords[qi, :3].tolist()}")


UNIFORM = [c for c in sc.CASES if c.thr != "mixed"]
MIXED = [c for c in sc.CASES if c.thr == "mixed"]


@pytest.mark.parametrize("case", UNIFORM, ids=[c.name for c in UNIFORM])
def test_skinny_case(case):
    """One case of the table through `search_device`; every run asserts the route and the instantiation that actually ran (`_assert_route`)."""
    torch = _torch()
    v, store, qs = sc.case_inputs(case)
    eng, dev = _engine(case, store)
    if case.group == "ladder" or any(sp > 0 for sp in case.splits):
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
            assert (np.sort(ords[:, : case.rows], axis=1) == np.arange(case.rows)[None, :]).all(), f"{case.name}: not the whole corpus"
    else:
        assert cnts[0] >= 1 and cnts.min() < case.k  # (sparse: the oracle decides each count)
    _check_oracle(case, v, qs, ords, scs, cnts, thrs)
    _check_planted(case, ords)
    if case.base:  # the base-0 keys with every ordinal shifted, scores bit for bit
        eng0, dev0 = _engine(case, store, base=0)
        base0 = eng0.search_device(dq, case.k, t32)
        eng0.synchronize()
        assert {g: eng0.get_option(g) for g in GETTERS} == {"last_tier": 5, "last_shadow": 0, "last_skinny_kernel": sc.kernel_id(case.dim, case.f32, 64)}
        np.testing.assert_array_equal(keys, sc.shift_keys(base0.cpu().numpy(), case.base), err_msg=case.name)
        assert int(ords.max()) + case.base <= 2**32 - 3
        eng0.close()
    if case.group == "qtail":
        # the queries next to the padding against their single lookups (the streaming kernels: another summation order, so the scores agree
        # within the project's score tolerance and no closer; the inputs have no near tie among these queries' best k + 1 rows)
        for name in ("skinny_min_batch_f16", "skinny_min_batch_f32"):
            eng.set_option(name, 1 << 20)
        for qi in sc.single_queries(case):
            so, ss = eng.search(qs[qi], case.k, np.float32(t32))
            assert eng.get_option("last_tier") in (1, 2, 3)
            m = int(cnts[qi])
            assert ords[qi, :m].tolist() == (np.asarray(so, dtype=np.int64) - case.base).tolist(), (case.name, qi)
            assert float(np.max(np.abs(scs[qi, :m].astype(np.float64) - np.asarray(ss, dtype=np.float64)))) <= vo.SCORE_TOL, (case.name, qi)
    eng.close()


@pytest.mark.parametrize("case", MIXED, ids=[c.name for c in MIXED])
def test_skinny_mixed_thresholds(case):
    """One threshold per query through `search_batch` (a NaN and a value above 1 among them): the same runs, identical answers, every live
    query against the oracle."""
    v, store, qs = sc.case_inputs(case)
    eng, dev = _engine(case, store)
    s0 = np.sort(vo.scores_full(v, qs[0]))[::-1]
    lo, hi = 0.0, float(s0[4])
    pattern = [lo, hi, float("nan"), 1.5, lo + (hi - lo) / 2]
    t = np.array([_native.f32_threshold(pattern[i % len(pattern)]) for i in range(case.nq)], dtype=np.float32)
    got = {}
    for run in sc.runs(case):
        eng.set_option("mfma_splits", run.splits)
        eng.set_option("mfma_sched", run.sched)
        ords, scs, cnts = eng.search_batch(qs[: run.nq], case.k, t[: run.nq])
        _assert_route(eng, case, run)
        for qi in range(run.nq):  # (slots past a query's count are not part of the answer)
            ords[qi, cnts[qi]:] = -1
            scs[qi, cnts[qi]:] = 0
        got[run] = (ords, scs, cnts)
    ords, scs, cnts = next(g for r, g in got.items() if r.nq == case.nq and r.sched == 0)
    for run, (o, s, c) in got.items():
        n = run.nq
        assert np.array_equal(c, cnts[:n]) and np.array_equal(o, ords[:n]) and np.array_equal(s.view(np.uint32), scs[:n].view(np.uint32)), (case.name, run.what)
    dead = np.isnan(t) | (t > 1)
    assert dead.any() and (cnts[dead] == 0).all()
    assert (cnts[t == 0] == case.k).all() and cnts[1] < case.k
    live = np.flatnonzero(~dead)
    for qi in live:
        m = int(cnts[qi])
        vo.check_topk_parity(vo.scores_full(v, qs[qi]), ords[qi, :m], scs[qi, :m], case.k, float(t[qi]), referee=vo.f64_referee(v, qs[qi]))
    eng.close()
