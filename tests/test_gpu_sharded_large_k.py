"""GPU suite: max_hits 257 .. 16384 on device groups and row-sharded indexes -- the merge of long sorted lists (tavb_merge_topk_device)
against the host merge, the device-resident large-k lookup (tavb_search_topk_device) against tavb_search_topk bit for bit, a device group
of three shards against one engine over the same rows, the collective forms on a forced one-rank communicator (chunking and fault
injection included) and two ranks on one GPU with the exchange over gloo.

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
from tests.synth import make_corpus, make_queries, subset_choice
from tests.test_sharded_large_k_host import FAILED, MERGE_SHAPES, make_lists
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

TEST_LIMIT_S = 420


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


# ---- the merge kernel -----------------------------------------------------------------------------------------------------------------

def test_merge_topk_device_equals_the_host_merge_in_both_layouts():
    import torch

    eng = _native.Engine(0)
    eng.profile_enable(True)
    eng.profile_reset()
    launches = 0
    for n_lists, k in MERGE_SHAPES + [(64, 5), (40, 7)]:
        rng = np.random.default_rng(1000 * n_lists + k)
        for nq, fill in ((1, "full"), (3, "ragged"), (2, "empty")):
            if k == 16384 and n_lists > 8 and fill != "full":
                continue
            lists = make_lists(rng, n_lists, nq, k, fill)
            if fill == "ragged":
                lists[0, 1, :] = FAILED  # one rank's lists of query 1: the failure key in every slot
                if n_lists > 1:
                    lists[n_lists - 1, 1, :] = FAILED  # ... and a second rank's: duplicated failure keys
            want = _native.merge_topk_keys(lists)
            dl = torch.from_numpy(lists.view(np.int64)).cuda()
            qm = dl.permute(1, 0, 2).contiguous()
            torch.cuda.synchronize()
            a = eng.merge_topk_device(dl)
            b = eng.merge_topk_device(qm, query_major=True)
            eng.synchronize()
            launches += 2
            np.testing.assert_array_equal(a.cpu().numpy().view(np.uint64), want, err_msg=f"{n_lists} x {nq} x {k} {fill}")
            np.testing.assert_array_equal(b.cpu().numpy().view(np.uint64), want, err_msg=f"query-major {n_lists} x {nq} x {k} {fill}")
            if fill == "ragged":
                assert (want[1] == FAILED).all() and (want[0] != FAILED).all()
    # straight into pinned host memory, as the collective calls write their answer
    lists = make_lists(np.random.default_rng(5), 8, 4, 1000, "ragged")
    pinned = torch.empty((4, 1000), dtype=torch.int64).pin_memory()
    dl = torch.from_numpy(lists.view(np.int64)).cuda()
    torch.cuda.synchronize()
    eng.merge_topk_device(dl, out_keys=pinned)
    eng.synchronize()
    np.testing.assert_array_equal(pinned.numpy().view(np.uint64), _native.merge_topk_keys(lists))
    assert eng.profile_read(_native.KERNEL_MERGE)[1] == launches + 1  # timed under TAVB_KERNEL_MERGE
    with pytest.raises(ValueError):
        eng.merge_topk_device(torch.zeros((65, 1, 4), dtype=torch.int64).cuda())
    eng.close()


# ---- tavb_search_topk_device ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("d", [100, 384, 1536, 3072])
def test_search_topk_device_equals_search_topk_bit_for_bit(dtype, d):
    import torch

    n, base = 20_011, 1000
    v, _ = make_corpus(n, d, 9300 + d)
    eng = _native.Engine(0)
    eng.ordinal_base = base
    eng.upload_rows(v, 0, _native.TAVB_F16 if dtype == "fp16" else _native.TAVB_F32)
    qs = make_queries(11, d, 9400 + d)  # two groups of the score pass
    thrs = np.asarray([0.0, 0.5, 0.52, 0.0, 0.49, 0.0, 0.7, 0.0, 0.51, 0.0, 2.0], dtype=np.float32)  # one threshold per query
    dq = torch.from_numpy(qs).cuda()
    rng = np.random.default_rng(d)
    rows = rng.integers(0, n, size=7000).astype(np.int64)  # a subset with duplicates
    drows = torch.from_numpy(rows.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    for k in (257, 1000, 16384):
        ords, scs, cnts = eng.search_topk(qs, k, thrs)
        assert ords[0, 0] >= base and cnts[10] == 0 and cnts[0] == min(k, n)
        keys = eng.search_topk_device(dq, k, thrs)
        eng.synchronize()
        assert eng.get_option("last_tier") in (1, 2, 3)
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), keys_of(ords, scs, cnts, k), err_msg=f"k={k}")
        # the subset form: positions
        pos, ps = eng.search_subset_topk(qs[1], rows, k, np.float32(0.3))
        skeys = eng.search_topk_device(dq[1:2], k, np.float32(0.3), dev_rows=drows)
        eng.synchronize()
        want = keys_of(pos[None, :], ps[None, :], [len(pos)], k)
        np.testing.assert_array_equal(skeys.cpu().numpy().view(np.uint64), want, err_msg=f"subset k={k}")
    # into pinned host memory
    pinned = torch.empty((11, 300), dtype=torch.int64).pin_memory()
    eng.search_topk_device(dq, 300, thrs, out_keys=pinned)
    eng.synchronize()
    np.testing.assert_array_equal(pinned.numpy().view(np.uint64), keys_of(*eng.search_topk(qs, 300, thrs), 300))
    with pytest.raises(ValueError):
        eng.search_topk_device(dq, _native.MAX_LARGE_K + 1, thrs)
    eng.close()


def test_search_topk_device_refines_a_corpus_of_identical_rows():
    import torch

    n = 40_000  # more rows in one score bucket than a boundary list holds: the refinement runs
    row, _ = make_corpus(1, 384, 9500)
    v = np.repeat(row, n, axis=0)
    eng = _native.Engine(0)
    eng.upload_rows(v, 0, _native.TAVB_F32)
    q = make_queries(2, 384, 9501)
    dq = torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    for k in (257, 5000):
        ords, scs, cnts = eng.search_topk(q, k, 0.0)
        host_rounds = eng.get_option("last_topk_refine")
        assert host_rounds > 0 and ords[0, :k].tolist() == list(range(k))
        keys = eng.search_topk_device(dq, k, 0.0)
        eng.synchronize()
        assert eng.get_option("last_topk_refine") == host_rounds
        np.testing.assert_array_equal(keys.cpu().numpy().view(np.uint64), keys_of(ords, scs, cnts, k))
    # "last_topk_refine" speaks of the LAST lookup: an asynchronous call that nobody waited for does not report over a later synchronous one
    eng.search_topk_device(dq, 257, 0.0)
    pos, _ = eng.search_subset_topk(q[0], np.arange(100, dtype=np.int64), 300, np.float32(0.0))  # 100 positions: nothing to refine
    assert len(pos) == 100 and eng.get_option("last_topk_refine") == 0
    eng.synchronize()
    assert eng.get_option("last_topk_refine") == 0
    eng.close()


def test_search_topk_device_on_an_empty_corpus_and_subset_gives_empty_lists():
    import torch

    v, _ = make_corpus(500, 384, 9600)
    eng = _native.Engine(0)
    eng.upload_rows(v, 0, _native.TAVB_F32)
    dq = torch.from_numpy(make_queries(2, 384, 9601)).cuda()
    none = torch.zeros(0, dtype=torch.int32).cuda()
    torch.cuda.synchronize()
    keys = eng.search_topk_device(dq[:1], 300, 0.0, dev_rows=none)
    eng.synchronize()
    assert (keys.cpu().numpy() == 0).all()
    eng.clear()
    keys = eng.search_topk_device(dq, 300, 0.0)
    eng.synchronize()
    assert (keys.cpu().numpy() == 0).all()
    eng.close()


# ---- a device group of three shards against ONE engine --------------------------------------------------------------------------------

def _device_list(n):
    have = _native.device_count()
    return [i % max(have, 1) for i in range(n)]


@pytest.mark.parametrize("dtype,d", [("fp32", 1536), ("fp16", 1536), ("fp16", 100), ("fp32", 100)])
def test_device_group_large_k_equals_one_engine_over_the_same_rows(dtype, d):
    n = 50_021
    v, q = make_corpus(n, d, 9700 + d)
    vv = _f16(v) if dtype == "fp16" else v
    group = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=_device_list(3), corpus_dtype=dtype)
    one = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    group.add_embeddings(None, v)
    one.add_embeddings(None, v)
    aligned = (d * (2 if dtype == "fp16" else 4)) % 16 == 0  # every shard starts on a 16-byte boundary: the same scan tier, the same arithmetic per row
    geng = group.engine
    geng.profile_enable(True)
    geng.profile_reset()
    res = group.fuzzy_lookup_embedding(q, max_hits=1000, min_score=0.0)
    # the route: the exact device top-k on EVERY shard, one score pass each, no emit-all pass
    assert len(geng.engines) == 3
    for e in geng.engines:
        assert e.profile_read(_native.KERNEL_TOPK)[1] >= 1 and e.profile_read(_native.KERNEL_SCAN)[1] == 1
        assert e.get_option("last_tier") in (1, 2, 3)
    assert len(res) == 1000 and max(r.item for r in res) > 2 * n // 3

    def check(got, want, scores, k, ms, candidates=None, rows=None, query=None):
        assert len(got) == len(want)
        if aligned:
            assert bits(got) == bits(want)
        else:  # a shard may start unaligned and take another scan tier: parity with the oracle, refereed in float64
            vo.check_topk_parity(scores, [r.item for r in got], [r.score for r in got], k, ms, candidate_ordinals=candidates,
                                 referee=vo.f64_referee(vv if rows is None else rows, query))

    check(res, one.fuzzy_lookup_embedding(q, max_hits=1000, min_score=0.0), vo.scores_full(vv, q), 1000, 0.0, query=q)
    qs = make_queries(40, d, 9800 + d)
    thr = [0.0 if i % 3 else 0.5 for i in range(40)]
    got = group.fuzzy_lookup_embeddings(qs, max_hits=300, min_score=thr)
    want = one.fuzzy_lookup_embeddings(qs, max_hits=300, min_score=thr)
    for i in range(40):
        check(got[i], want[i], vo.scores_full(vv, qs[i]), 300, thr[i], query=qs[i])
    sub = subset_choice(n, 9000, 9900 + d) + [7, 7, -1, -n, 12_345, 12_345]
    sub_a = np.asarray(sub, dtype=np.int64)
    got = group.fuzzy_lookup_embedding_in_subset(q, sub, max_hits=500, min_score=0.0)
    want = one.fuzzy_lookup_embedding_in_subset(q, sub, max_hits=500, min_score=0.0)
    assert len(got) == 500
    check(got, want, vo.scores_full(vv, q)[sub_a], 500, 0.0, candidates=sub_a, rows=vv[sub_a], query=q)
    # the switch: "large_k" = 0 brings the emit-all route back
    geng.set_option("large_k", 0)
    geng.profile_reset()
    old = group.fuzzy_lookup_embedding(q, max_hits=1000, min_score=0.0)
    for e in geng.engines:
        assert e.profile_read(_native.KERNEL_TOPK)[1] == 0 and e.profile_read(_native.KERNEL_SCAN)[1] == 1
    assert bits(old) == bits(res)
    geng.set_option("large_k", 1)
    # what the route does not take keeps the emit-all pass: every survivor, and more hits than TAVB_MAX_LARGE_K
    geng.profile_reset()
    every = group.fuzzy_lookup_embedding(q, max_hits=0, min_score=0.55)
    assert all(e.profile_read(_native.KERNEL_TOPK)[1] == 0 for e in geng.engines)
    want = one.fuzzy_lookup_embedding(q, max_hits=0, min_score=0.55)
    assert len(every) == len(want) and (not aligned or bits(every) == bits(want))
    geng.profile_enable(False)


# ---- the collective forms on a forced one-rank communicator ---------------------------------------------------------------------------

def test_collective_large_k_on_a_forced_one_rank_communicator():
    import torch

    from typeagent_py_amd.sharded import DeviceShardBackend, PeerFailedError, ShardedSearcher, ShardedVectorBase

    n, d, k, nq = 30_001, 384, 1000, 5
    v, _ = make_corpus(n, d, 9950)
    qs = make_queries(nq, d, 9951)
    thrs = np.asarray([0.0, 0.5, 0.0, 0.51, 0.0], dtype=np.float32)
    backend = DeviceShardBackend(0)
    with torch.cuda.stream(backend.stream):
        shard = torch.from_numpy(v).cuda()
    backend.set_shard(shard, row_offset=7_000)
    dq = torch.from_numpy(qs).cuda()
    torch.cuda.synchronize()
    eng = backend.engine
    plain = eng.search_topk_device(dq, k, thrs)
    eng.synchronize()
    plain = plain.cpu().numpy().view(np.uint64)
    assert (plain[0] != 0).all()
    eng.profile_enable(True)

    def join(reserve):
        if reserve is not None:
            eng.set_option("comm_reserve_keys", reserve)  # (read by tavb_comm_init)
        backend.init_comm(0, 1)
        eng.set_option("comm_force", 1)
        eng.profile_reset()

    # 1. the lists fit the reserve: one all-gather, one merge
    join(None)
    pinned = torch.empty((nq, k), dtype=torch.int64).pin_memory()
    eng.search_topk_allgather(dq, k, thrs, out_keys=pinned)
    eng.synchronize()
    np.testing.assert_array_equal(pinned.numpy().view(np.uint64), plain)
    assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == 1 and eng.profile_read(_native.KERNEL_MERGE)[1] == 1
    assert eng.profile_read(_native.KERNEL_TOPK)[1] >= 1
    merged = eng.allgather_merge_topk(torch.from_numpy(plain.view(np.int64)).to("cuda"))  # the exchange on its own
    eng.synchronize()
    np.testing.assert_array_equal(merged.cpu().numpy().view(np.uint64), plain)
    # the front ends ride it: plain, batched and subset lookups at max_hits 1000 against the oracle
    backend.set_shard(shard, row_offset=0)
    svb = ShardedVectorBase(backend, 0, n, n)
    before = eng.profile_read(_native.KERNEL_EXCHANGE)[1]
    hits = svb.fuzzy_lookup_embedding(qs[0], max_hits=k, min_score=0.0)
    vo.check_topk_parity(vo.scores_full(v, qs[0]), [h.item for h in hits], [h.score for h in hits], k, 0.0, referee=vo.f64_referee(v, qs[0]))
    sub = np.random.default_rng(3).integers(-40, n, size=6000).tolist() + [5, 5]
    sub_a = np.asarray(sub, dtype=np.int64)
    got = svb.fuzzy_lookup_embedding_in_subset(qs[1], sub, max_hits=k, min_score=0.0)
    assert len(got) == k
    vo.check_topk_parity(vo.scores_full(v, qs[1])[sub_a], [h.item for h in got], [h.score for h in got], k, 0.0, candidate_ordinals=sub_a,
                         referee=vo.f64_referee(v[sub_a], qs[1]))
    assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 2
    for bad in (0, 20000):
        with pytest.raises(ValueError, match="1..16384"):
            svb.fuzzy_lookup_embedding(qs[0], max_hits=bad)
    backend.set_shard(shard, row_offset=7_000)
    eng.comm_destroy()

    # 2. a reserve below the call's lists (5 x 1000 keys against 2048): three chunks of whole queries, the same answer
    join(2048)
    pinned.zero_()
    eng.search_topk_allgather(dq, k, thrs, out_keys=pinned)
    eng.synchronize()
    np.testing.assert_array_equal(pinned.numpy().view(np.uint64), plain)
    assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == 3 and eng.profile_read(_native.KERNEL_MERGE)[1] == 3
    # a list that does not fit the reserve at all is an argument error every rank makes alike
    with pytest.raises(ValueError, match="comm_reserve_keys"):
        eng.search_topk_allgather(dq, 4096, thrs)
    # 3. fault injection: the rank's own error, the exchange still runs, the output leads with the failure key
    searcher = ShardedSearcher(backend)
    for option, value, off, message in (("comm_fail_rank", 0, -1, "injected failure of the local search"),
                                        ("comm_fail_alloc", 1, 0, "injected failure of the list allocation")):
        before = eng.profile_read(_native.KERNEL_EXCHANGE)[1]
        eng.set_option(option, value)
        pinned.zero_()
        with pytest.raises(_native.TavbError, match=message):
            eng.search_topk_allgather(dq, k, thrs, out_keys=pinned)
        eng.synchronize()
        assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 3  # every chunk of the exchange was joined
        assert (pinned.numpy().view(np.uint64)[:, 0] == FAILED).all()
        with pytest.raises(_native.TavbError, match="rank of the collective lookup failed"):
            _native.decode_keys(pinned.numpy())
        with pytest.raises((_native.TavbError, PeerFailedError)):
            searcher.search(dq, k, 0.0)
        eng.set_option(option, off)
    res = searcher.search(dq, k, 0.0)  # and the next lookup lines up
    assert int(res.counts[0]) == k
    eng.comm_destroy()
    eng.profile_enable(False)


# ---- two ranks on one GPU, the exchange over gloo -------------------------------------------------------------------------------------

N2, D2, K2 = 30_001, 384, 1000


def _two_rank_worker(rank, world, port, ret):
    import torch
    import torch.distributed as dist

    faulthandler.dump_traceback_later(TEST_LIMIT_S - 60, exit=True)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from typeagent_py_amd.sharded import DeviceShardBackend, ShardedSearcher, ShardedVectorBase, shard_range

        v, _ = make_corpus(N2, D2, 9960)
        qs = make_queries(3, D2, 9961)
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

        searcher = ShardedSearcher(backend, gather_fn=gather_over_gloo)
        dq = torch.from_numpy(qs).cuda()
        torch.cuda.synchronize()
        res = searcher.search(dq, K2, 0.0)
        svb = ShardedVectorBase(backend, lo, hi - lo, len(v))
        svb.searcher.gather_fn = gather_over_gloo
        sub = np.random.default_rng(4).integers(-30, N2, size=5000).tolist()
        got = svb.fuzzy_lookup_embedding_in_subset(qs[1], sub, max_hits=K2, min_score=0.0)
        ret[rank] = (res.ordinals.copy(), res.scores.copy(), res.counts.copy(), [(h.item, h.score) for h in got])
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_large_k_equals_the_whole_corpus():
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    v, _ = make_corpus(N2, D2, 9960)
    qs = make_queries(3, D2, 9961)
    for qi in range(3):
        np.testing.assert_array_equal(ret[0][0][qi], ret[1][0][qi])
        np.testing.assert_array_equal(ret[0][1][qi], ret[1][1][qi])
        assert int(ret[0][2][qi]) == K2
        vo.check_topk_parity(vo.scores_full(v, qs[qi]), ret[0][0][qi].tolist(), ret[0][1][qi].tolist(), K2, 0.0, referee=vo.f64_referee(v, qs[qi]))
    assert ret[0][0].max() > N2 // 2  # hits from the second shard carry their global ordinals
    assert ret[0][3] == ret[1][3] and len(ret[0][3]) == K2
    sub_a = np.asarray(np.random.default_rng(4).integers(-30, N2, size=5000), dtype=np.int64)
    vo.check_topk_parity(vo.scores_full(v, qs[1])[sub_a], [i for i, _ in ret[0][3]], [s_ for _, s_ in ret[0][3]], K2, 0.0, candidate_ordinals=sub_a,
                         referee=vo.f64_referee(v[sub_a], qs[1]))
