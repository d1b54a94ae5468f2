"""GPU suite: masked lookups on device groups and row-sharded indexes -- the no-wait batched subset call
(tavb_search_subset_batch_device) against the host-synchronous one (tavb_search_subset_batch_resident) bit for bit, a device group of
three shards against its own per-query fallback and the oracle, the collective form on a forced one-rank communicator, and two ranks on
one GPU with the exchange over gloo.

Every test runs under a watchdog of its own (a test that hangs ends the whole run: nothing more is started on the GPU) and nothing is
retried."""

import faulthandler
import os
import socket
import sys

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import RowMask, TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

TEST_LIMIT_S = 300


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def keys_of(ords, scs, cnts, k):
    """(ordinals, scores, counts) of a host lookup -> the packed, zero-padded keys the device forms write"""
    nq = len(cnts)
    keys = np.zeros((nq, k), dtype=np.uint64)
    for q in range(nq):
        m = int(cnts[q])
        keys[q, :m] = (scs[q, :m].astype(np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ords[q, :m].astype(np.uint64))
    return keys


def bits(res):
    return [r.item for r in res], np.asarray([r.score for r in res], dtype=np.float32).view(np.uint32).tolist()


# ---- tavb_search_subset_batch_device ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [100, 384, 1536])
def test_subset_batch_device_equals_subset_batch_resident_bit_for_bit(dtype, d):
    import torch

    n, base = 20_011, 1000
    v, _ = make_corpus(n, d, 11300 + d)
    eng = _native.Engine(0)
    eng.ordinal_base = base
    eng.upload_rows(v, 0, _native.TAVB_F16 if dtype == "fp16" else _native.TAVB_F32)
    qs = make_queries(11, d, 11400 + d)  # two groups of queries (three at k > 64)
    thrs = np.asarray([0.0, 0.5, 0.52, 0.0, 0.49, 0.0, 0.7, 0.0, 0.51, 0.0, 2.0], dtype=np.float32)  # one threshold per query
    dq = torch.from_numpy(qs).cuda()
    mask = np.random.default_rng(d).random(n) < 0.5
    half, count = eng.mask_to_rows(mask)
    assert count == int(mask.sum())
    seven = torch.from_numpy(np.asarray([3, 17, 4096, 9000, 16384, 20_000, n - 1], dtype=np.int32)).cuda()
    torch.cuda.synchronize()
    for rows in (half, seven):
        for k in (10, 256, 257, 1000):
            pinned = torch.empty((11, k), dtype=torch.int64).pin_memory()
            for remap in (0, 1):
                ords, scs, cnts = eng.search_subset_batch_resident(qs, rows, k, thrs, remap=bool(remap))
                assert cnts[10] == 0 and cnts[0] == min(k, len(rows))
                assert ords[0, 0] >= (base if remap else 0) and (remap or ords[0, : cnts[0]].max() < len(rows))
                want = keys_of(ords, scs, cnts, k)
                keys = eng.search_subset_batch_device(dq, rows, k, thrs, remap=bool(remap))
                pinned.fill_(-1)
                eng.search_subset_batch_device(dq, rows, k, thrs, out_keys=pinned, remap=bool(remap))
                eng.synchronize()
                what = f"rows={len(rows)} k={k} remap={remap}"
                np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), want, err_msg=what)
                np.testing.assert_array_equal(pinned.numpy().view(np.uint64), want, err_msg="pinned " + what)
    for bad_k in (0, _native.MAX_LARGE_K + 1):
        with pytest.raises(ValueError):
            eng.search_subset_batch_device(dq, half, bad_k, thrs)
    eng.close()


def test_subset_batch_device_empty_lists_and_ties():
    import torch

    row, _ = make_corpus(1, 384, 11500)
    v = np.repeat(row, 3000, axis=0)  # identical rows: every score ties
    eng = _native.Engine(0)
    eng.ordinal_base = 50
    eng.upload_rows(v, 0, _native.TAVB_F32)
    dq = torch.from_numpy(make_queries(9, 384, 11501)).cuda()
    rows = torch.arange(5, 3000, 3, dtype=torch.int32).cuda()
    none = torch.zeros(0, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    for k in (10, 300):
        keys = eng.search_subset_batch_device(dq, rows, k, 0.0, remap=True)
        eng.synchronize()
        ords, _, cnts = _native.decode_keys(keys.cpu().numpy())
        assert (cnts == k).all()
        for q in range(9):
            assert ords[q].tolist() == [50 + 5 + 3 * i for i in range(k)]  # ties come back in ascending ordinal order
        pos = eng.search_subset_batch_device(dq, rows, k, 0.0, remap=False)
        eng.synchronize()
        assert _native.decode_keys(pos.cpu().numpy())[0][0].tolist() == list(range(k))
        for remap in (False, True):  # an empty row list: all-zero keys, in device memory and in pinned memory
            out = torch.full((9, k), -1, dtype=torch.int64).cuda()
            pinned = torch.full((9, k), -1, dtype=torch.int64).pin_memory()
            torch.cuda.synchronize()
            eng.search_subset_batch_device(dq, none, k, 0.0, out_keys=out, remap=remap)
            eng.search_subset_batch_device(dq, none, k, 0.0, out_keys=pinned, remap=remap)
            eng.synchronize()
            assert (out.cpu().numpy() == 0).all() and (pinned.numpy() == 0).all()
    eng.clear()  # an empty corpus
    for k in (10, 300):
        keys = eng.search_subset_batch_device(dq, rows, k, 0.0)
        eng.synchronize()
        assert (keys.cpu().numpy() == 0).all()
    eng.close()


# ---- a device group of three shards ----------------------------------------------------------------------------------------------------

N_GROUP = 50_021
GROUP_SHAPES = [("fp32", 384), ("fp16", 384), ("fp16", 100), ("fp32", 100)]
GROUP_MASKS = ["random_0.5", "random_0.01", "all", "none", "no_shard_1", "one_in_last", "boundaries"]
GROUP_NQS = [1, 9, 17]
GROUP_HITS = [10, 256, 300]
THR_CYCLE = [0.0, 0.5, 0.6, 0.45, 1.5, -0.2, 0.55, 0.52]
_groups: dict = {}


def _device_list(n):
    have = _native.device_count()
    return [i % max(have, 1) for i in range(n)]


def group_setup(dtype, d):
    """(index over three shards, the rows as the kernels see them, queries, their scores over every row) -- built once per shape"""
    key = (dtype, d)
    if key not in _groups:
        v, _ = make_corpus(N_GROUP, d, 11700 + d)
        qs = make_queries(max(GROUP_NQS), d, 11800 + d)
        qs[3] = v[N_GROUP // 2]  # a query equal to a row: something passes 0.6
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=_device_list(3), corpus_dtype=dtype)
        vb.add_embeddings(None, v)
        vv = _f16(v) if dtype == "fp16" else v
        geng = vb.engine
        assert len(geng.engines) == 3 and geng.masked_capable()
        bounds = list(geng.bounds)
        assert all(b % 32 for b in bounds[1:]) and all(hi - lo > _native.MASK_ROWS_PER_WORKGROUP for lo, hi in zip(bounds, bounds[1:]))
        _groups[key] = (vb, vv, qs, [vo.cosine_to_score(np.dot(vv, q)) for q in qs])
    return _groups[key]


def group_mask(kind, bounds):
    n = bounds[-1]
    m = np.zeros(n, dtype=bool)
    if kind.startswith("random_"):
        m = np.random.default_rng(n + 11).random(n) < float(kind.split("_")[1])
        m[n // 2] = True
    elif kind == "all":
        m[:] = True
    elif kind == "no_shard_1":
        m = np.random.default_rng(n + 12).random(n) < 0.3
        m[bounds[1] : bounds[2]] = False
    elif kind == "one_in_last":
        m[bounds[2] + 4321] = True
    elif kind == "boundaries":
        for b in bounds[1:-1]:
            m[b - 1] = m[b] = True
        m[0] = m[n - 1] = True
    return m


@pytest.mark.parametrize("k", GROUP_HITS)
@pytest.mark.parametrize("kind", GROUP_MASKS)
@pytest.mark.parametrize("dtype,d", GROUP_SHAPES)
def test_device_group_masked_equals_its_fallback_and_the_oracle(dtype, d, kind, k):
    import torch

    vb, vv, qs, scores = group_setup(dtype, d)
    geng = vb.engine
    mask = group_mask(kind, list(geng.bounds))
    flat = np.flatnonzero(mask)
    aligned = (d * (2 if dtype == "fp16" else 4)) % 16 == 0  # every shard's rows start on a 16-byte boundary: one scan tier for both routes
    handle = vb.row_mask(mask)
    assert isinstance(handle, RowMask) and handle.count == len(flat) and handle.rows == N_GROUP and handle.shards is not None
    assert [h is not None for h in handle.shards] == [bool(mask[lo:hi].any()) for lo, hi in zip(geng.bounds, geng.bounds[1:])]
    np.testing.assert_array_equal(handle.flat(), flat)
    every = [mask, handle, torch.from_numpy(mask).to("cuda:0")]  # an array, a RowMask, a torch.bool tensor on device 0
    # one form per batch size, in turn; the sparse and the boundary mask (cheap to referee) cross every form with every batch size
    forms = {nq: every if kind in ("random_0.01", "boundaries") else [every[i]] for i, nq in enumerate(GROUP_NQS)}
    sub = vv[flat]
    referees = [vo.f64_referee(sub, q) for q in qs]
    sub_scores = [s[flat] for s in scores]
    for ms in (0.0, "per_query"):
        thr = (lambda i: THR_CYCLE[i % len(THR_CYCLE)]) if ms == "per_query" else (lambda i: ms)
        seq = [vb.fuzzy_lookup_embedding_in_subset(q, flat, max_hits=k, min_score=thr(i)) for i, q in enumerate(qs)] if len(flat) else [[]] * len(qs)
        for nq in reversed(GROUP_NQS):
            arg = [thr(i) for i in range(nq)] if ms == "per_query" else ms
            for form, i in [(f, i) for f in forms[nq] for i in range(nq)]:
                if i == 0:
                    got = vb.fuzzy_lookup_embeddings_masked(qs[:nq], form, max_hits=k, min_score=arg)
                    assert len(got) == nq
                what = (kind, k, ms, nq, i)
                if len(flat) == 0:
                    assert got[i] == [], what
                    continue
                assert len(got[i]) == len(seq[i]), what
                if aligned:
                    assert bits(got[i]) == bits(seq[i]), what
                if not aligned or nq == max(GROUP_NQS):  # (aligned: the smaller batches are the fallback's lists bit for bit, like the largest, refereed here)
                    vo.check_topk_parity(sub_scores[i], [r.item for r in got[i]], [r.score for r in got[i]], k, thr(i), candidate_ordinals=flat,
                                         referee=referees[i])
        if k <= 256 and ms == "per_query":  # as_arrays agrees with the lists
            arg = [thr(i) for i in range(9)]
            lists = vb.fuzzy_lookup_embeddings_masked(qs[:9], handle, max_hits=k, min_score=arg)
            ords, scs, cnts = vb.fuzzy_lookup_embeddings_masked(qs[:9], handle, max_hits=k, min_score=arg, as_arrays=True)
            assert ords.shape == scs.shape == (9, k) and cnts.tolist() == [len(h) for h in lists]
            for i, hits in enumerate(lists):
                assert ords[i, : cnts[i]].tolist() == [h.item for h in hits]
                assert scs[i, : cnts[i]].view(np.uint32).tolist() == bits(hits)[1]


def test_device_group_masked_route_and_the_large_k_switch():
    """The route by its launches: a 17-query lookup at max_hits 10 is what ONE engine over one shard's rows runs for a batched resident
    subset lookup of 17 queries (ceil(17 / TAVB_MAX_STREAM_QUERIES) scans and merges, no selection pass) on every shard that has allowed
    rows and nothing on the shard that has none; the fallback would scan 17 times per shard."""
    vb, vv, qs, scores = group_setup("fp32", 384)
    geng = vb.engine
    bounds = list(geng.bounds)
    mask = group_mask("no_shard_1", bounds)
    flat = np.flatnonzero(mask)
    handle = vb.row_mask(mask)
    counters = (_native.KERNEL_SCAN, _native.KERNEL_MERGE, _native.KERNEL_TOPK)
    # the expectation: a single engine holding shard 0's rows, the batched resident subset lookup over shard 0's part of the mask
    one = _native.Engine(0)
    one.upload_rows(vv[: bounds[1]], 0, _native.TAVB_F32)
    rows0, _ = one.mask_to_rows(mask[: bounds[1]])
    expect = {}
    for k in (10, 300):
        one.profile_enable(True)
        one.profile_reset()
        one.search_subset_batch_resident(qs, rows0, k, 0.0)
        expect[k] = [one.profile_read(c)[1] for c in counters]
    one.close()
    per_pass = -(-17 // _native.MAX_STREAM_QUERIES)
    assert expect[10] == [per_pass, per_pass, 0] and expect[300][0] >= 1 and expect[300][2] >= 1
    geng.profile_enable(True)
    try:
        for k in (10, 300):
            geng.profile_reset()
            got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=0.0)
            assert [[e.profile_read(c)[1] for c in counters] for e in geng.engines] == [expect[k], [0, 0, 0], expect[k]], k
            assert all(len(hits) == k for hits in got)
        # the fallback for comparison: one scan per query and shard
        geng.profile_reset()
        seq = [vb.fuzzy_lookup_embedding_in_subset(q, flat, max_hits=10, min_score=0.0) for q in qs]
        assert [e.profile_read(_native.KERNEL_SCAN)[1] for e in geng.engines] == [17, 0, 17]
        got = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=10, min_score=0.0)
        assert [bits(a) for a in got] == [bits(b) for b in seq]
        # "large_k" off: max_hits 300 goes back to the per-query fallback (no selection pass anywhere), with the same answers
        on = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=300, min_score=0.0)
        geng.set_option("large_k", 0)
        geng.profile_reset()
        off = vb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=300, min_score=0.0)
        assert all(e.profile_read(_native.KERNEL_TOPK)[1] == 0 for e in geng.engines)
        assert [e.profile_read(_native.KERNEL_SCAN)[1] for e in geng.engines] == [17, 0, 17]
        assert [bits(a) for a in off] == [bits(b) for b in on]
    finally:
        geng.set_option("large_k", 1)
        geng.profile_enable(False)


# ---- the collective form on a forced one-rank communicator -----------------------------------------------------------------------------

def test_sharded_masked_on_a_forced_one_rank_communicator():
    import torch

    from typeagent_py_amd.sharded import DeviceShardBackend, ShardedVectorBase

    n, d, nq = 30_001, 384, 5
    v, _ = make_corpus(n, d, 11950)
    qs = make_queries(nq, d, 11951)
    thrs = [0.0, 0.5, 0.0, 0.51, 0.0]
    backend = DeviceShardBackend(0)
    with torch.cuda.stream(backend.stream):
        shard = torch.from_numpy(v).cuda()
    backend.set_shard(shard, row_offset=0)
    torch.cuda.synchronize()
    eng = backend.engine
    backend.init_comm(0, 1)
    eng.set_option("comm_force", 1)
    eng.profile_enable(True)
    eng.profile_reset()
    svb = ShardedVectorBase(backend, 0, n, n)
    mask = np.random.default_rng(6).random(n) < 0.4
    flat = np.flatnonzero(mask)
    sub = v[flat]
    try:
        # a mask made by kernels on the CALLER's stream right before row_mask (a fresh scope: timestamps > t0), behind work that keeps
        # that stream busy: the handle is of the finished mask
        stamps = np.random.default_rng(7).random(n).astype(np.float32)
        dev_stamps = torch.from_numpy(stamps).to("cuda:0")
        busy = torch.full((4096, 4096), 1e-3, device="cuda:0")
        torch.cuda.synchronize()
        for _ in range(24):
            busy = busy @ busy
        fresh = svb.row_mask(dev_stamps > 0.6)
        want = np.flatnonzero(stamps > 0.6)
        assert fresh.count == len(want)
        np.testing.assert_array_equal(fresh.flat(), want)
        np.testing.assert_array_equal(fresh.dev_rows.cpu().numpy(), want)
        for _ in range(24):
            busy = busy @ busy
        part = backend.mask_to_device(dev_stamps > 0.3)
        np.testing.assert_array_equal(part.cpu().numpy(), np.flatnonzero(stamps > 0.3))
        del busy
        for form in (mask, torch.from_numpy(mask).to("cuda:0")):
            handle = svb.row_mask(form)
            assert handle.count == len(flat) and handle.dev_rows is not None and handle.layout == (n, 0, n)
            np.testing.assert_array_equal(handle.flat(), flat)
            for k in (10, 1000):
                before = eng.profile_read(_native.KERNEL_EXCHANGE)[1]
                got = svb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=thrs)
                assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 1  # ONE exchange for the batch (the fallback: one per query)
                for i in range(nq):
                    vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [h.item for h in got[i]], [h.score for h in got[i]], k, thrs[i],
                                         candidate_ordinals=flat, referee=vo.f64_referee(sub, qs[i]))
                assert len(got[0]) == k
                again = [svb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=thrs) for _ in range(2)]  # the handle reused
                assert again[0] == got and again[1] == got
                assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 3
        for bad in (0, 20000):
            with pytest.raises(ValueError, match="1..16384"):
                svb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=bad)
    finally:
        eng.comm_destroy()
        eng.profile_enable(False)


# ---- two ranks on one GPU, the exchange over gloo --------------------------------------------------------------------------------------

N2, D2 = 30_001, 384


def _two_rank_masks():
    rng = np.random.default_rng(11)
    both = rng.random(N2) < 0.3
    upper = both.copy()
    upper[: N2 // 2 + 1] = False  # nothing allowed in rank 0's part
    return both, upper


def _two_rank_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist

    faulthandler.dump_traceback_later(TEST_LIMIT_S - 60, exit=True)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from typeagent_py_amd.sharded import DeviceShardBackend, ShardedVectorBase, shard_range

        v, _ = make_corpus(N2, D2, 11960)
        qs = make_queries(3, D2, 11961)
        lo, hi = shard_range(len(v), world, rank)
        backend = DeviceShardBackend(0)  # both ranks share GPU 0; RCCL refuses that, so the exchange goes over gloo
        with torch.cuda.stream(backend.stream):
            shard = torch.from_numpy(v[lo:hi]).cuda()
        backend.set_shard(shard, row_offset=lo)

        def gather_over_gloo(local):
            backend.stream.synchronize()
            host = local.cpu()
            parts = [torch.empty_like(host) for _ in range(world)]
            dist.all_gather(parts, host)
            return torch.stack(parts).contiguous().cuda()

        svb = ShardedVectorBase(backend, lo, hi - lo, len(v))
        svb.searcher.gather_fn = gather_over_gloo
        out = []
        for mask in _two_rank_masks():
            handle = svb.row_mask(mask)
            for k in (10, 300):
                got = svb.fuzzy_lookup_embeddings_masked(qs, handle, max_hits=k, min_score=[0.0, 0.5, 0.0])
                out.append([[(h.item, h.score) for h in hits] for hits in got])
        ret[rank] = (out, handle.dev_rows is None)
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_masked_equals_the_whole_corpus():
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    v, _ = make_corpus(N2, D2, 11960)
    qs = make_queries(3, D2, 11961)
    assert ret[0][0] == ret[1][0]  # both ranks return the same lists
    assert ret[0][1] is True and ret[1][1] is False  # the second mask left rank 0's part empty: it joined all the same
    case = 0
    for mask in _two_rank_masks():
        flat = np.flatnonzero(mask)
        sub = v[flat]
        for k in (10, 300):
            got = ret[0][0][case]
            case += 1
            for i, ms in enumerate([0.0, 0.5, 0.0]):
                vo.check_topk_parity(vo.cosine_to_score(np.dot(sub, qs[i])), [o for o, _ in got[i]], [s_ for _, s_ in got[i]], k, ms,
                                     candidate_ordinals=flat, referee=vo.f64_referee(sub, qs[i]))
            assert len(got[0]) == k
            assert max(o for o, _ in got[0]) > N2 // 2  # hits from the second shard carry global ordinals
