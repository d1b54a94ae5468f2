"""Large-k lookups (max_hits 257 .. 16384) on device groups and row shards: three markdown tables, the source of
profiles/r10_sharded_large_k.md.

  group       VectorBase(devices=[0, 0, 0]) -- a device group of three shards on ONE GPU -- at max_hits 1000 and 4096 over 10k fp32, 1M fp32
              and 10M fp16 rows (1536 wide), one query and 32: the new route (tavb_search_topk_device per shard, tavb_merge_topk_host)
              against the emit-all route it replaces ("large_k" = 0 in the same process), legs interleaved, medians of --reps
              host-synchronous calls, answers compared bit for bit
  merge       tavb_merge_topk_device alone (event time, TAVB_KERNEL_MERGE) for n_lists 2 / 4 / 8 x k 1000 / 16384 x nq 1 / 64, as a fraction of
              the local top-k of the same call (score pass + selection, TAVB_KERNEL_SCAN + TAVB_KERNEL_TOPK, 1M fp16 rows), next to a sort of
              the union of the lists (tavb_sort_keys_device, one host-synchronous call per query: one workgroup in LDS up to 16384 keys, the
              radix sort beyond), wall time against the merge's wall time -- a stand-in built from parts that exist, NOT the bisection + LDS
              sort candidate, which was not built
  collective  tavb_search_topk_allgather on a forced one-rank communicator against tavb_search_topk_device over the same rows: what the
              exchange and the merge add, host-synchronous medians and event times

  python tools/sharded_large_k_sweep.py [--parts group,merge,collective] [--sizes 10k,1m,10m] [--reps 21]
"""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import host_queries, make_device_corpus  # noqa: E402
from tests.fakes import NullModel  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402

SIZES = {"10k": (10_000, "fp32"), "1m": (1_000_000, "fp32"), "10m": (10_000_000, "fp16")}
DIM = 1536


def interleaved(legs, reps):
    """legs: name -> callable; every round runs every leg once, in turn -> (name -> median ms, name -> last result)"""
    out = {name: fn() for name, fn in legs.items()}  # warm-up (workspaces, pinned buffers, LDS attributes)
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            out[name] = fn()
            ts[name].append(time.perf_counter() - t0)
    return {name: float(np.median(t)) * 1e3 for name, t in ts.items()}, out


def pairs(res):
    return [([r.item for r in q], np.asarray([r.score for r in q], np.float32).view(np.uint32).tolist()) for q in res]


def device_corpus(rows, dtype, seed):
    eng = _native.Engine(0)
    corpus = make_device_corpus(eng, rows, DIM, seed, dtype)
    eng.close()
    return corpus


def part_group(sizes, reps):
    print("\n### Device group of 3 shards on one GPU: new route against emit-all (`large_k` = 0)\n")
    print("| corpus | nq | max_hits | new ms | emit-all ms | emit-all / new | bit-identical |")
    print("|---|---|---|---|---|---|---|")
    for size in sizes:
        rows, dtype = SIZES[size]
        corpus = device_corpus(rows, dtype, 4242 + rows % 1000)
        cuts = [rows * i // 3 for i in range(4)]
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 0, 0], corpus_dtype=dtype)
        vb.adopt_device_corpus([corpus[cuts[i] : cuts[i + 1]] for i in range(3)])
        eng = vb.engine
        for nq in (1, 32):
            qs = host_queries(nq, DIM, 99 + nq)
            for k in (1000, 4096):
                def call(on):
                    eng.set_option("large_k", on)
                    if nq == 1:
                        return [vb.fuzzy_lookup_embedding(qs[0], max_hits=k, min_score=0.0)]
                    return vb.fuzzy_lookup_embeddings(qs, max_hits=k, min_score=0.0)

                ms, out = interleaved({"new": lambda: call(1), "old": lambda: call(0)}, reps)
                eng.set_option("large_k", 1)
                same = pairs(out["new"]) == pairs(out["old"])
                print(f"| {size} {dtype} | {nq} | {k} | {ms['new']:.3f} | {ms['old']:.3f} | {ms['old'] / ms['new']:.2f} | {'yes' if same else 'NO'} |", flush=True)
        del vb, eng, corpus


def part_merge(reps):
    import torch

    print("\n### The merge kernel alone (1M fp16 rows per list's shard; event times per call)\n")
    print("| n_lists | k | nq | local top-k ms (events) | merge ms (events) | merge / local | merge, host-synchronous call ms | sort of the union, nq host-synchronous calls ms |")
    print("|---|---|---|---|---|---|---|---|")
    rows = 1_000_000
    corpus = device_corpus(rows, "fp16", 777)
    eng = _native.Engine(0)
    eng.profile_enable(True)
    for nq in (1, 64):
        dq = torch.from_numpy(host_queries(nq, DIM, 31 + nq)).to("cuda:0")
        torch.cuda.synchronize()
        for k in (1000, 16384):
            for n_lists in (2, 4, 8):
                lists = torch.empty((n_lists, nq, k), dtype=torch.int64, device="cuda:0")
                for i in range(n_lists):  # the same rows under another ordinal base: unique keys, every list full
                    eng.set_corpus_tensor(corpus, ordinal_base=i * rows)
                    eng.search_topk_device(dq, k, 0.0, out_keys=lists[i])
                eng.synchronize()
                eng.profile_reset()
                for _ in range(reps):
                    eng.search_topk_device(dq, k, 0.0, out_keys=lists[n_lists - 1])
                eng.synchronize()
                local = (eng.profile_read(_native.KERNEL_SCAN)[0] + eng.profile_read(_native.KERNEL_TOPK)[0]) / reps
                out = torch.empty((nq, k), dtype=torch.int64, device="cuda:0")
                eng.merge_topk_device(lists, out_keys=out)
                eng.profile_reset()
                for _ in range(reps):
                    eng.merge_topk_device(lists, out_keys=out)
                eng.synchronize()
                merge = eng.profile_read(_native.KERNEL_MERGE)[0] / reps
                walls = []
                for _ in range(reps):  # the same merge as a host-synchronous call: what the sort below can be set against
                    t0 = time.perf_counter()
                    eng.merge_topk_device(lists, out_keys=out)
                    eng.synchronize()
                    walls.append(time.perf_counter() - t0)
                union = lists.permute(1, 0, 2).contiguous().view(nq, n_lists * k)
                ts = []
                for _ in range(max(3, reps // 4)):
                    work = union.clone()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for q in range(nq):
                        eng.sort_keys_device(work[q])  # (returns after the sort has finished)
                    ts.append(time.perf_counter() - t0)
                # the sort orders the keys as unsigned values, as the merge does: the same best k
                assert torch.equal(work[:, :k], out), "the merge and the sort of the union disagree"
                print(f"| {n_lists} | {k} | {nq} | {local:.3f} | {merge:.3f} | {merge / local:.3f} | {float(np.median(walls)) * 1e3:.3f} | "
                      f"{float(np.median(ts)) * 1e3:.3f} |", flush=True)
    eng.close()


def part_collective(reps):
    import torch

    from typeagent_py_amd.sharded import DeviceShardBackend

    print("\n### Forced one-rank collective against the local lookup (1M fp16 rows)\n")
    print("| nq | k | search_topk_device ms | search_topk_allgather ms | added ms | exchange event ms | merge event ms | identical |")
    print("|---|---|---|---|---|---|---|---|")
    rows = 1_000_000
    corpus = device_corpus(rows, "fp16", 778)
    backend = DeviceShardBackend(0)
    backend.set_shard(corpus, row_offset=0)
    backend.init_comm(0, 1)
    eng = backend.engine
    eng.set_option("comm_force", 1)
    eng.profile_enable(True)
    for nq in (1, 32):
        dq = torch.from_numpy(host_queries(nq, DIM, 57 + nq)).to("cuda:0")
        torch.cuda.synchronize()
        for k in (1000, 4096, 16384):
            a = torch.empty((nq, k), dtype=torch.int64).pin_memory()
            b = torch.empty((nq, k), dtype=torch.int64).pin_memory()

            def local():
                eng.search_topk_device(dq, k, 0.0, out_keys=a)
                eng.synchronize()

            def coll():
                eng.search_topk_allgather(dq, k, 0.0, out_keys=b)
                eng.synchronize()

            local()
            coll()
            eng.profile_reset()
            ms, _ = interleaved({"local": local, "coll": coll}, reps)
            n = reps + 1
            ex, mg = eng.profile_read(_native.KERNEL_EXCHANGE)[0] / n, eng.profile_read(_native.KERNEL_MERGE)[0] / n
            print(f"| {nq} | {k} | {ms['local']:.3f} | {ms['coll']:.3f} | {ms['coll'] - ms['local']:.3f} | {ex:.3f} | {mg:.3f} | "
                  f"{'yes' if torch.equal(a, b) else 'NO'} |", flush=True)
    eng.comm_destroy()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="group,merge,collective")
    ap.add_argument("--sizes", default="10k,1m,10m")
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    parts = [p for p in args.parts.split(",") if p]
    if "merge" in parts:
        part_merge(args.reps)
    if "collective" in parts:
        part_collective(args.reps)
    if "group" in parts:
        part_group([s for s in args.sizes.split(",") if s], args.reps)


if __name__ == "__main__":
    main()
