"""Masked lookups over shards: a device group of three shards on ONE GPU (default 1M x 1536 fp16 rows) and the row-sharded form on a forced
one-rank communicator, at mask densities 1 %, 10 % and 50 %, for 1, 8 and 32 queries at max_hits 10.

  cut+expand  VectorBase.row_mask(numpy mask) on the group: the mask cut at the shard bounds, every slice packed, uploaded and expanded on
              its shard's device (tavb_mask_expand) -- paid once per mask
  masked      fuzzy_lookup_embeddings_masked(Q queries, RowMask): one tavb_search_subset_batch_device per shard, merged on the host
  fallback    [fuzzy_lookup_embedding_in_subset(q, np.flatnonzero(mask)) for q in queries]: what the same call did before the group had a
              route of its own (the parent commit's behaviour, forced in the same process on the same box)
  sharded     ShardedVectorBase.fuzzy_lookup_embeddings_masked over the same rows as ONE shard with the communicator forced on: one local
              call, ONE exchange -- against Q subset lookups (Q exchanges), the fallback of that class

The legs of a cell run interleaved (masked, fallback, masked, ...); medians of host-synchronous calls in ms; answers compared bit for bit.
Writes a markdown report (default profiles/r13_masked_shards.md).

  python tools/masked_shards_sweep.py [--rows 1000000] [--dtype fp16] [--densities 0.01,0.1,0.5] [--nqs 1,8,32] [--k 10] [--reps 9] [--out ...]
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


def interleaved(legs: dict, reps: int):
    """legs: name -> callable; every round runs every leg once, in turn -> (name -> median ms, name -> last result)"""
    out = {name: fn() for name, fn in legs.items()}  # warm-up (workspaces, pinned buffers, the subset cache)
    ts = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            out[name] = fn()
            ts[name].append(time.perf_counter() - t0)
    return {name: float(np.median(t)) * 1e3 for name, t in ts.items()}, out


def pairs(res):
    return [([r.item for r in q], np.asarray([r.score for r in q], np.float32).view(np.uint32).tolist()) for q in res]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--densities", default="0.01,0.1,0.5")
    ap.add_argument("--nqs", default="1,8,32")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_masked_shards.md"))
    args = ap.parse_args()
    import torch

    from typeagent_py_amd.sharded import DeviceShardBackend, ShardedVectorBase

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    rows, k = args.rows, args.k
    nqs = [int(x) for x in args.nqs.split(",")]
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, rows, args.dim, 4242, args.dtype)
    eng0.close()
    cuts = [rows * i // 3 for i in range(4)]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 0, 0], corpus_dtype=args.dtype)
    vb.adopt_device_corpus([corpus[cuts[i] : cuts[i + 1]] for i in range(3)])
    backend = DeviceShardBackend(0)
    backend.set_shard(corpus, row_offset=0)
    backend.init_comm(0, 1)
    backend.engine.set_option("comm_force", 1)
    svb = ShardedVectorBase(backend, 0, rows, rows)
    qs = host_queries(max(nqs), args.dim, 131)
    lines = [
        "# Masked lookups on a device group and on a row-sharded index",
        "",
        "`" + " ".join(["python", "tools/masked_shards_sweep.py"] + shown) + "`",
        "",
        f"{rows} x {args.dim} {args.dtype} rows on one MI355X ({torch.cuda.get_device_name(0)}), max_hits = {k}, min_score = 0, medians of {args.reps} host-synchronous calls, ms;",
        "the legs of a cell interleaved.  `fallback` = one `fuzzy_lookup_embedding_in_subset` per query over `np.flatnonzero(mask)`: what the masked",
        "lookups of these two classes did before they had a route of their own, forced in the same process.",
        "",
        "- The numbers come from ONE GPU hosting all three shards of the group (and the one rank of the communicator): the shards' kernels share",
        "  that GPU, so what several devices gain by scanning concurrently is not in them.",
        "- Two or more real GPUs are unmeasured: no box of the pool shows a second one.",
        "",
        "## Device group of three shards",
        "",
        "| density | rows allowed | cut+expand | nq | masked | fallback | fallback / masked | bit-identical |",
        "|---|---|---|---|---|---|---|---|",
    ]
    sharded_lines = [
        "",
        "## Row-sharded index, one rank, communicator forced on",
        "",
        "| density | rows allowed | row_mask | nq | masked (1 exchange) | nq subset lookups (nq exchanges) | subset / masked | bit-identical |",
        "|---|---|---|---|---|---|---|---|",
    ]
    for dens in (float(x) for x in args.densities.split(",")):
        mask = np.random.default_rng(int(dens * 1000)).random(rows) < dens
        flat = np.flatnonzero(mask)
        t_cut, out = interleaved({"cut": lambda: vb.row_mask(mask)}, max(3, args.reps // 3))
        handle = out["cut"]
        t_smask, out = interleaved({"cut": lambda: svb.row_mask(mask)}, max(3, args.reps // 3))
        shandle = out["cut"]
        for nq in nqs:
            legs = {"masked": lambda: vb.fuzzy_lookup_embeddings_masked(qs[:nq], handle, k, 0.0),
                    "fallback": lambda: [vb.fuzzy_lookup_embedding_in_subset(q, flat, k, 0.0) for q in qs[:nq]]}
            ms, res = interleaved(legs, args.reps)
            ok = pairs(res["masked"]) == pairs(res["fallback"])
            lines.append(f"| {dens:g} | {len(flat)} | {t_cut['cut']:.3f} | {nq} | {ms['masked']:.3f} | {ms['fallback']:.3f} | {ms['fallback'] / ms['masked']:.2f} | {'yes' if ok else 'NO'} |")
            print(lines[-1], flush=True)
            legs = {"masked": lambda: svb.fuzzy_lookup_embeddings_masked(qs[:nq], shandle, k, 0.0),
                    "fallback": lambda: [svb.fuzzy_lookup_embedding_in_subset(q, flat, k, 0.0) for q in qs[:nq]]}
            ms, res = interleaved(legs, args.reps)
            ok = pairs(res["masked"]) == pairs(res["fallback"])
            sharded_lines.append(f"| {dens:g} | {len(flat)} | {t_smask['cut']:.3f} | {nq} | {ms['masked']:.3f} | {ms['fallback']:.3f} | {ms['fallback'] / ms['masked']:.2f} | {'yes' if ok else 'NO'} |")
            print(sharded_lines[-1], flush=True)
    backend.engine.comm_destroy()
    text = "\n".join(lines + sharded_lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
