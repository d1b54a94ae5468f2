"""GPU suite: top-k distinct messages on device groups and row-sharded indexes -- the device merge of top-messages lists
(tavb_merge_top_messages_device) against the host merge bit for bit, a device group of three shards against the same group on the host
collapse and against a single-GPU index, the route by its launch counters, the collective form on a forced one-rank communicator, and two
ranks on one GPU with the exchange over gloo.

Every test runs under a watchdog of its own (a test that hangs ends the whole run: nothing more is started on the GPU) and nothing is
retried."""

import faulthandler
import os
import socket
import sys

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import top_messages_shards_cases as tc
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu

TEST_LIMIT_S = 300


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _f16(v):
    return v.astype(np.float16).astype(np.float32)


def bits(res):
    return [r.item for r in res], np.asarray([r.score for r in res], dtype=np.float32).view(np.uint32).tolist()


# ---- tavb_merge_top_messages_device ----------------------------------------------------------------------------------------------------

MERGE_SHAPES = [(n, k) for k in (1, 10, 300, 16384) for n in (1, 3, 8)] + [(64, 10)]
_engine: list = []


def merge_engine():
    if not _engine:
        _engine.append(_native.Engine(0))
    return _engine[0]


def device_merge(eng, lists: np.ndarray, n_messages: int, query_major: bool, pinned: bool) -> np.ndarray:
    import torch

    n_lists, nq, k = lists.shape
    host = np.ascontiguousarray(lists.transpose(1, 0, 2) if query_major else lists).view(np.int64)
    dev = torch.from_numpy(host).cuda()
    out = torch.full((nq, k), -7, dtype=torch.int64)
    out = out.pin_memory() if pinned else out.cuda()
    torch.cuda.synchronize()
    got = eng.merge_top_messages_device(dev, n_messages, out_keys=out, query_major=query_major)
    eng.synchronize()
    return got.cpu().numpy().view(np.uint64) if not pinned else got.numpy().view(np.uint64).copy()


@pytest.mark.parametrize("n_lists,k", MERGE_SHAPES)
def test_device_merge_of_top_messages_lists_equals_the_host_merge_bit_for_bit(n_lists, k):
    eng = merge_engine()
    rng = np.random.default_rng(100 * n_lists + k)
    for n_messages in (5, 1000, 100003):
        for nq in (1, 9):  # nine queries: a second sub-group
            lists = tc.random_lists(rng, n_lists, nq, k, "ragged" if nq == 9 else "full", n_messages)
            lists[0, 0, 0] = tc.make_keys([1.0], [n_messages - 1])[0]  # the last message, at the best score
            if nq == 9:
                lists[n_lists - 1, 4, :] = tc.FAILED  # a failed list fails its query and only it
            want = _native.merge_top_messages_keys(lists)
            np.testing.assert_array_equal(want, tc.merge_statement(lists))
            for query_major, pinned in ((False, False), (True, True)) if k == 16384 else ((False, False), (False, True), (True, False), (True, True)):
                got = device_merge(eng, lists, n_messages, query_major, pinned)
                np.testing.assert_array_equal(got, want, err_msg=f"n_messages={n_messages} nq={nq} query_major={query_major} pinned={pinned}")
            if nq == 9:
                assert (want[4] == tc.FAILED).all() and (want[:4] != tc.FAILED).all()


def test_device_merge_drops_keys_beyond_n_messages_and_refuses_bad_shapes():
    import torch

    eng = merge_engine()
    k, n_messages = 10, 1000
    lists = np.zeros((2, 1, k), dtype=np.uint64)
    lists[0, 0, :3] = tc.make_keys([0.9, 0.8, 0.7], [n_messages, 5, n_messages - 1])  # message 1000 is beyond: dropped, never written
    lists[1, 0, :3] = tc.make_keys([0.95, 0.6, 0.5], [2_000_000_000, 5, 7])
    inside = lists.copy()
    inside[0, 0, :3] = [lists[0, 0, 1], lists[0, 0, 2], 0]
    inside[1, 0, :3] = [lists[1, 0, 1], lists[1, 0, 2], 0]
    for query_major in (False, True):
        got = device_merge(eng, lists, n_messages, query_major, False)
        np.testing.assert_array_equal(got, _native.merge_top_messages_keys(inside))
        assert tc.decoded(got[0])[0] == [5, n_messages - 1, 7]
    dev = torch.zeros((2, 1, k), dtype=torch.int64).cuda()
    for bad in (0, -3, 2**31 - 1):
        with pytest.raises((ValueError, _native.TavbError)):  # (an argument error is a ValueError, "unsupported" a TavbError)
            eng.merge_top_messages_device(dev, bad)
    with pytest.raises(ValueError):
        eng.merge_top_messages_device(torch.zeros((65, 1, k), dtype=torch.int64).cuda(), 10)


def test_device_merge_one_query_per_sub_group_and_equal_scores_around_the_boundary():
    eng = merge_engine()
    rng = np.random.default_rng(8)
    n_messages = 5000
    lists = tc.random_lists(rng, 3, 9, 300, "full", n_messages)
    want = _native.merge_top_messages_keys(lists)
    floor = eng.get_option("topk_scores_bytes")
    eng.set_option("topk_scores_bytes", 4096)  # the option's floor: one query per sub-group
    try:
        np.testing.assert_array_equal(device_merge(eng, lists, n_messages, False, False), want)
    finally:
        eng.set_option("topk_scores_bytes", floor)
    # 600 messages at ONE score around rank 300, split over three lists that overlap: the boundary bucket holds more keys than the
    # boundary list of the selection takes, so it is refined
    cap = eng.get_option("topk_boundary_keys")
    eng.set_option("topk_boundary_keys", 64)
    try:
        k = 300
        tie = np.zeros((3, 1, k), dtype=np.uint64)
        for l in range(3):
            msgs = np.concatenate([np.arange(l * 10, l * 10 + 20), 100 + np.arange(l * 200, l * 200 + 280) % 600])
            scs = np.concatenate([np.full(20, 0.9, np.float32), np.full(280, 0.5, np.float32)])
            tie[l, 0] = np.sort(tc.make_keys(scs, msgs))[::-1]
        want = _native.merge_top_messages_keys(tie)
        np.testing.assert_array_equal(want, tc.merge_statement(tie))
        np.testing.assert_array_equal(device_merge(eng, tie, 1000, False, True), want)
        assert eng.get_option("last_topk_refine") > 0
    finally:
        eng.set_option("topk_boundary_keys", cap)


# ---- a device group of three shards ----------------------------------------------------------------------------------------------------

N_GROUP = 20_011
GROUP_SHAPES = [("fp32", 384), ("fp16", 384), ("fp16", 100), ("fp16", 1536)]
_groups: dict = {}


def _device_list(n):
    have = _native.device_count()
    return [i % max(have, 1) for i in range(n)]


def group_setup(dtype, d):
    """(index over three shards, single-GPU index over the same rows, the rows as the kernels see them, queries) -- built once per shape"""
    key = (dtype, d)
    if key not in _groups:
        v, _ = make_corpus(N_GROUP, d, 12700 + d)
        qs = make_queries(max(tc.NQS), d, 12800 + d)
        qs[3] = v[N_GROUP // 2]  # a query equal to a row: something passes 0.6
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=_device_list(3), corpus_dtype=dtype)
        vb.add_embeddings(None, v)
        one = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
        one.add_embeddings(None, v)
        geng = vb.engine
        assert len(geng.engines) == 3 and geng.masked_capable() and geng.top_messages_capable()
        assert all(b % 3 for b in geng.bounds[1:-1])  # messages of 3 chunks straddle the shard bounds
        _groups[key] = (vb, one, _f16(v) if dtype == "fp16" else v, qs)
    return _groups[key]


def message_oracle(vv, q, mapping, mask):
    """(message ordinals, per message the oracle's best float32 score and the best float64 score) over the allowed rows that have a message"""
    allowed = (mapping >= 0) if mask is None else (mask & (mapping >= 0))
    rows = np.flatnonzero(allowed)
    rows = rows[np.argsort(mapping[rows], kind="stable")]
    msgs, starts = np.unique(mapping[rows], return_index=True)
    s32 = vo.cosine_to_score(np.dot(vv[rows], q))
    s64 = vo.f64_referee(vv[rows], q)(np.arange(len(rows)))
    return msgs, np.maximum.reduceat(s32, starts), np.maximum.reduceat(s64, starts)


def check_against_the_oracle(oracle, k, thr, got):
    """the 100-wide fp16 rows: a shard's rows do not start on the 16-byte boundary the whole corpus' do, so the scan tier and with it the
    last bits of a score may differ -- the oracle's scores collapsed in numpy, near-ties refereed in float64"""
    msgs, best32, best64 = oracle
    vo.check_topk_parity(best32, [h.item for h in got], [h.score for h in got], k, thr, score_tol=vo.SCORE_TOL, candidate_ordinals=msgs,
                         referee=lambda pos: best64[pos])


def check_every_message(oracle, thr, got):
    """K above the message count: the answer is EVERY message with a passing row, so nothing can be swapped over rank K.  Each returned
    score is within SCORE_TOL of the oracle's best for that message, the list descends and names no message twice, every message whose
    float64 best clears the threshold by more than SCORE_TOL is there and none that misses it by more is.  (The checker of the other
    depths is quadratic in K; a few queries take it at this depth too.)"""
    msgs, best32, best64 = oracle
    items = np.asarray([h.item for h in got], dtype=np.int64)
    scores = np.asarray([h.score for h in got], dtype=np.float32)
    assert len(set(items.tolist())) == len(items) and (np.diff(scores) <= 0).all()
    at = np.searchsorted(msgs, items)
    assert (at < len(msgs)).all() and (msgs[at] == items).all()
    assert (np.abs(scores.astype(np.float64) - best64[at]) <= vo.SCORE_TOL).all()
    present = np.zeros(len(msgs), dtype=bool)
    present[at] = True
    assert present[best64 >= thr + vo.SCORE_TOL].all() and not present[best64 < thr - vo.SCORE_TOL].any()


AB_LEGS = {(9, 10), (1, 300), (17, 1)}  # (queries, K) at which the same group answers on the host collapse as well: "top_messages" = 0


@pytest.mark.parametrize("map_kind", tc.MAPS)
@pytest.mark.parametrize("dtype,d", GROUP_SHAPES)
def test_device_group_top_messages_equals_the_host_collapse_and_one_gpu(dtype, d, map_kind):
    vb, one, vv, qs = group_setup(dtype, d)
    geng = vb.engine
    bounds = list(geng.bounds)
    mapping = tc.message_map(N_GROUP, map_kind)
    n_messages = int(mapping.max()) + 1
    vb.set_row_messages(mapping)
    one.set_row_messages(mapping)
    aligned = (d * (2 if dtype == "fp16" else 4)) % 16 == 0
    most = max(tc.NQS)
    for mask_kind in tc.MASKS:
        mask = tc.group_mask(mask_kind, bounds)
        handle = None if mask is None else vb.row_mask(mask)
        handle_one = None if mask is None else one.row_mask(mask)
        oracles = [] if aligned else [message_oracle(vv, qs[i], mapping, mask) for i in range(most)]  # (once per mask, shared)
        for k in tc.ks_for(n_messages):
            for thr_kind in tc.THRESHOLDS:
                largest = None
                for nq in sorted(tc.NQS, reverse=True):
                    what = (mask_kind, nq, k, thr_kind)
                    thrs = tc.thresholds(thr_kind, nq)
                    got = vb.lookup_top_messages_by_embeddings(qs[:nq], k, thrs, allowed=handle)
                    assert len(got) == nq, what
                    if thr_kind == "nothing":
                        assert got == [[] for _ in range(nq)], what
                        continue
                    if aligned:
                        want = one.lookup_top_messages_by_embeddings(qs[:nq], k, thrs, allowed=handle_one)
                        assert [bits(a) for a in got] == [bits(b) for b in want], what
                    else:
                        # every query of the largest batch against the oracle; a query of a smaller batch whose list is the largest
                        # batch's bit for bit (the thresholds are the same per query) has been checked there, any other is checked here
                        if largest is None:
                            largest = got
                        for i in range(nq):
                            if got is not largest and bits(got[i]) == bits(largest[i]):
                                continue
                            thr = tc.threshold_of(thr_kind, i)
                            if k > n_messages:
                                check_every_message(oracles[i], thr, got[i])
                            if k <= n_messages or (nq == 9 and i in (0, 3)) or got is not largest:
                                check_against_the_oracle(oracles[i], k, thr, got[i])
                    if aligned and ((nq, k) in AB_LEGS or (k > n_messages and nq == 1)):  # the A/B leg: the same group on the host collapse
                        geng.set_option("top_messages", 0)
                        try:
                            off = vb.lookup_top_messages_by_embeddings(qs[:nq], k, thrs, allowed=handle)
                        finally:
                            geng.set_option("top_messages", 1)
                        assert [bits(a) for a in got] == [bits(b) for b in off], what
    if map_kind == "chunks3":
        assert len(vb.lookup_top_messages_by_embedding(qs[0], n_messages + 5, 0.0)) == n_messages  # K above the message count: every message


def test_device_group_top_messages_route_by_its_launches_and_the_switch():
    """On every shard with allowed rows exactly what ONE engine over that shard's rows records for `search_top_messages` over its part of
    the mask; nothing on a shard without allowed rows; with "top_messages" = 0 the host collapse's emit-all route and the same answers."""
    vb, one_gpu, vv, qs = group_setup("fp32", 384)
    geng = vb.engine
    bounds = list(geng.bounds)
    mapping = tc.message_map(N_GROUP, "interleaved")
    vb.set_row_messages(mapping)
    mask = tc.group_mask("no_shard_1", bounds)
    handle = vb.row_mask(mask)
    counters = (_native.KERNEL_SCAN, _native.KERNEL_MERGE, _native.KERNEL_TOPK)
    one = _native.Engine(0)
    one.upload_rows(vv[: bounds[1]], 0, _native.TAVB_F32)
    one.set_row_messages(mapping[: bounds[1]], int(mapping.max()) + 1)
    rows0, _ = one.mask_to_rows(mask[: bounds[1]])
    expect = {}
    for k in (10, 300):
        one.profile_enable(True)
        one.profile_reset()
        one.search_top_messages(qs, k, 0.0, dev_rows=rows0)
        expect[k] = [one.profile_read(c)[1] for c in counters]
        assert expect[k][0] >= 1 and expect[k][1] == 0 and expect[k][2] >= 1
    one.close()
    geng.profile_enable(True)
    try:
        for k in (10, 300):
            geng.profile_reset()
            got = vb.lookup_top_messages_by_embeddings(qs, k, 0.0, allowed=handle)
            assert [[e.profile_read(c)[1] for c in counters] for e in geng.engines] == [expect[k], [0, 0, 0], expect[k]], k
            assert all(len(hits) == k for hits in got)
        on = vb.lookup_top_messages_by_embeddings(qs, 10, 0.0, allowed=handle)
        geng.set_option("top_messages", 0)
        geng.profile_reset()
        off = vb.lookup_top_messages_by_embeddings(qs, 10, 0.0, allowed=handle)
        launches = [[e.profile_read(c)[1] for c in counters] for e in geng.engines]
        assert launches[1] == [0, 0, 0] and launches[0] != expect[10] and launches[0][0] >= 1  # the old route: not the top-messages passes
        assert [bits(a) for a in off] == [bits(b) for b in on]
    finally:
        geng.set_option("top_messages", 1)
        geng.profile_enable(False)


def test_device_group_top_messages_after_row_edits_and_scoped():
    d = 384
    v, _ = make_corpus(6_007, d, 12900)
    qs = make_queries(5, d, 12901)
    mapping = tc.message_map(len(v), "chunks3")
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=_device_list(3))
    vb.add_embeddings(None, v)
    vb.set_row_messages(mapping)
    first = vb.lookup_top_messages_by_embeddings(qs, 10, 0.0)
    gone = np.arange(100, 2500, 7)
    vb.remove_rows(gone)
    extra, _ = make_corpus(50, d, 12902)
    vb.insert_rows(1000, extra, row_messages=np.arange(5000, 5050))
    keep = np.delete(np.arange(len(v)), gone)
    rows = np.concatenate([v[keep][:1000], extra, v[keep][1000:]])
    msgs = np.concatenate([mapping[keep][:1000], np.arange(5000, 5050), mapping[keep][1000:]])
    fresh = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    fresh.add_embeddings(None, rows)
    fresh.set_row_messages(msgs)
    for k in (10, 300):
        got = vb.lookup_top_messages_by_embeddings(qs, k, [0.0, 0.5, 0.0, 0.45, 0.0])
        want = fresh.lookup_top_messages_by_embeddings(qs, k, [0.0, 0.5, 0.0, 0.45, 0.0])
        assert [bits(a) for a in got] == [bits(b) for b in want]
    assert all(len(hits) == 10 for hits in first)
    # one scope per query: the group loops over the one-mask call, every iteration on the new route
    rng = np.random.default_rng(4)
    scopes = [rng.random(len(rows)) < p for p in (0.5, 0.02, 0.5, 0.9, 0.3)]
    got = vb.lookup_top_messages_by_embeddings_scoped(qs, scopes, 10, 0.0)
    want = fresh.lookup_top_messages_by_embeddings_scoped(qs, scopes, 10, 0.0)
    assert [bits(a) for a in got] == [bits(b) for b in want]


# ---- the collective form on a forced one-rank communicator -----------------------------------------------------------------------------

def test_sharded_top_messages_on_a_forced_one_rank_communicator():
    import torch

    from typeagent_py_amd.sharded import DeviceShardBackend, ShardedVectorBase

    n, d, nq = 30_001, 384, 5
    v, _ = make_corpus(n, d, 12950)
    qs = make_queries(nq, d, 12951)
    thrs = [0.0, 0.5, 0.0, 0.51, 0.0]
    mapping = tc.message_map(n, "chunks3")
    one = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    one.add_embeddings(None, v)
    one.set_row_messages(mapping)
    backend = DeviceShardBackend(0)
    with torch.cuda.stream(backend.stream):
        shard = torch.from_numpy(v).cuda()
    backend.set_shard(shard, row_offset=0)
    torch.cuda.synchronize()
    eng = backend.engine
    mask = np.random.default_rng(6).random(n) < 0.4
    try:
        backend.init_comm(0, 1)
        eng.set_option("comm_force", 1)
        eng.profile_enable(True)
        eng.profile_reset()
        svb = ShardedVectorBase(backend, 0, n, n)
        svb.set_row_messages(mapping)
        for allowed in (None, mask):
            handle = None if allowed is None else svb.row_mask(allowed)
            handle_one = None if allowed is None else one.row_mask(allowed)
            for k in (10, 1000):
                before = eng.profile_read(_native.KERNEL_EXCHANGE)[1]
                got = svb.lookup_top_messages_by_embeddings(qs, k, thrs, allowed=handle)
                assert eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 1  # ONE exchange for the batch
                want = one.lookup_top_messages_by_embeddings(qs, k, thrs, allowed=handle_one)
                assert [bits(a) for a in got] == [bits(b) for b in want]
                assert len(got[0]) == k
                again = svb.lookup_top_messages_by_embeddings(qs, k, thrs, allowed=handle)  # the handle reused
                assert again == got and eng.profile_read(_native.KERNEL_EXCHANGE)[1] == before + 2
        assert svb.lookup_top_messages_by_embedding(qs[1], 10, 0.5) == svb.lookup_top_messages_by_embeddings(qs[1:2], 10, 0.5)[0]
        for bad in (0, 20000):
            with pytest.raises(ValueError, match="1..16384"):
                svb.lookup_top_messages_by_embeddings(qs, max_messages=bad)
    finally:
        eng.comm_destroy()
        eng.profile_enable(False)


# ---- two ranks on one GPU, the exchange over gloo --------------------------------------------------------------------------------------

N2, D2 = 30_001, 384


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

        v, _ = make_corpus(N2, D2, 12960)
        qs = make_queries(3, D2, 12961)
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
        for kind in ("chunks3", "interleaved"):  # (the cut at 15001 is no multiple of 3: a message straddles it)
            svb.set_row_messages(tc.message_map(N2, kind))
            for k in (10, 300):
                got = svb.lookup_top_messages_by_embeddings(qs, k, [0.0, 0.5, 0.0])
                out.append([[(h.item, float(np.float32(h.score).view(np.uint32))) for h in hits] for hits in got])
        ret[rank] = out
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_top_messages_equals_the_whole_corpus():
    import torch.multiprocessing as mp

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_two_rank_worker, args=(2, port, ret), nprocs=2, join=True)
    assert ret[0] == ret[1]  # both ranks return the same lists
    v, _ = make_corpus(N2, D2, 12960)
    qs = make_queries(3, D2, 12961)
    one = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0)
    one.add_embeddings(None, v)
    case = 0
    for kind in ("chunks3", "interleaved"):
        one.set_row_messages(tc.message_map(N2, kind))
        for k in (10, 300):
            want = one.lookup_top_messages_by_embeddings(qs, k, [0.0, 0.5, 0.0])
            got = ret[0][case]
            case += 1
            assert [([m for m, _ in hits], [int(b) for _, b in hits]) for hits in got] == [bits(w) for w in want]
            assert len(got[0]) == k
