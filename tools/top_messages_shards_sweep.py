"""Top-k distinct messages on a device group: `lookup_top_messages_by_embeddings` on `VectorBase(devices=[0, 0, 0])` -- three row shards on
ONE GPU, each running tavb_search_top_messages_device, merged by tavb_merge_top_messages_host -- against the route it replaces (engine
option "top_messages" = 0 on the group: the all-survivor lookup on every shard and a collapse on the host), in one process, on one corpus
(default 1M x 1536, fp16 and fp32), for 3 and 8 chunks per message, 1 / 8 / 32 queries, max_messages 25 / 1000, threshold 0 and a
threshold about 1 % of the rows pass, unmasked and under 10 / 50 % random masks.  Beside the two routes, per cell: the host merge alone
(`merge_top_messages_keys` over the three shards' lists) and the forced one-rank collective (`ShardedVectorBase` over the whole corpus with
"comm_force": search, all-gather, device merge in one C call); per (max_messages, queries): the device merge alone
(`Engine.merge_top_messages_device` over three random lists at --merge-messages message counts).

The legs are interleaved -- every round times each leg (median of --reps host-synchronous calls) in turn -- and a cell reports the median
over --rounds rounds, `old / new` (above 1 the new route wins) and the spread of the old route's rounds ((max - min) / median): a new route
slower than the old one by more than that spread is listed.  Answers are compared bit for bit between the legs.  `--max-host-rows` skips
the old route where it would build more than that many hit objects per call (queries x passing rows; 0 = no limit).  Three shards on one
GPU serialise on its CUs: what two or more real GPUs give is NOT measured by this tool.  Writes a markdown report; whatever the report
file already holds from the line `KEEP` on is carried over unchanged.

  python tools/top_messages_shards_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--reps 3] [--rounds 3] [--out profiles/r28_top_messages_shards.md]
  python tools/top_messages_shards_sweep.py --quick     (100k rows, fp16, one mask: a few seconds)
"""

from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import host_queries, make_device_corpus  # noqa: E402
from tests.fakes import NullModel  # noqa: E402
from tools.scoped_batch_sweep import KEEP, kept_tail, median_ms, same  # noqa: E402,F401
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402
from typeagent_py_amd.sharded import DeviceShardBackend, ShardedVectorBase  # noqa: E402


def random_lists(rng, n_lists: int, nq: int, k: int, n_messages: int) -> np.ndarray:
    """int64 [n_lists, nq, k]: sorted lists of min(k, n_messages) keys, one per message within a list, messages shared between the lists"""
    lists = np.zeros((n_lists, nq, k), dtype=np.uint64)
    m = min(k, n_messages)
    for l in range(n_lists):
        for q in range(nq):
            bits = rng.random(m).astype(np.float32).view(np.uint32).astype(np.uint64)
            keys = (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rng.choice(n_messages, size=m, replace=False).astype(np.uint64))
            lists[l, q, :m] = np.sort(keys)[::-1]
    return lists.view(np.int64)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--chunks", default="3,8")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--ks", default="25,1000")
    ap.add_argument("--masks", default="none,10%,50%")
    ap.add_argument("--merge-messages", default="333334,125000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-host-rows", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_top_messages_shards.md"))
    args = ap.parse_args()
    if args.quick:
        args.rows, args.dtypes, args.masks, args.chunks = min(args.rows, 100_000), "fp16", "none,10%", "3"
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    props = torch.cuda.get_device_properties(0)
    lines = [
        "# Top-k distinct messages on a device group of three shards on one GPU",
        "",
        "`" + " ".join(["python", "tools/top_messages_shards_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)} ({props.multi_processor_count} CUs), three row shards on ONE GPU,",
        "host-synchronous calls, ms.  `new` = `lookup_top_messages_by_embeddings` on the group with `top_messages` = 1 (one",
        "tavb_search_top_messages_device per shard + tavb_merge_top_messages_host); `old` = the same call with `top_messages` = 0 (the parent",
        "commit's route: every survivor of every shard sorted, copied out and collapsed on the host); `host merge` = the merge of the three",
        "shards' lists alone; `collective` = `ShardedVectorBase` over the whole corpus on a forced one-rank communicator (search, all-gather and",
        f"device merge in one C call).  {args.rounds} rounds of (median of {args.reps} calls) per leg, legs interleaved; `spread` = (max - min) / median of",
        "the old route's rounds.  Two or more real GPUs are NOT measured here: three shards on one GPU take turns on its CUs.",
        "",
        "| dtype | chunks / message | mask | threshold | max_messages | queries | passing | new | old | old / new | spread | slower beyond the spread | host merge | collective | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells, skipped = [], []
    for dtype in args.dtypes.split(","):
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        cut = [0, -(-args.rows // 3), min(args.rows, 2 * -(-args.rows // 3)), args.rows]
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), devices=[0, 0, 0], corpus_dtype=dtype)
        vb.adopt_device_corpus([corpus[a:b] for a, b in zip(cut, cut[1:])])
        geng = vb.engine
        backend = DeviceShardBackend(0)
        backend.set_shard(corpus, row_offset=0)
        backend.init_comm(0, 1)
        backend.engine.set_option("comm_force", 1)
        svb = ShardedVectorBase(backend, 0, args.rows, args.rows)
        qs = host_queries(32, args.dim, 131)
        rng = np.random.default_rng(77)
        masks = {"none": None, "10%": rng.random(args.rows) < 0.1, "50%": rng.random(args.rows) < 0.5}
        # a threshold that about 1 % of the rows pass for query 0
        sample = [h.score for h in vb.fuzzy_lookup_embedding(qs[0], max(args.rows // 100, 1), 0.0)]
        one_pct = float(sample[-1]) if sample else 0.0
        try:
            for chunks in (int(x) for x in args.chunks.split(",")):
                mapping = np.arange(args.rows, dtype=np.int64) // chunks
                vb.set_row_messages(mapping)
                svb.set_row_messages(mapping)
                for mask in args.masks.split(","):
                    allowed = None if masks[mask] is None else vb.row_mask(masks[mask])
                    allowed_s = None if masks[mask] is None else svb.row_mask(masks[mask])
                    for thr in (0.0, one_pct):
                        geng.set_option("top_messages", 1)
                        passing = int(args.rows * (1.0 if masks[mask] is None else masks[mask].mean()) * (1.0 if thr == 0.0 else 0.01))
                        for k in (int(x) for x in args.ks.split(",")):
                            for nq in (int(x) for x in args.batches.split(",")):
                                label = f"{dtype}, {chunks} chunks, mask {mask}, threshold {thr:g}, max_messages {k}, {nq} queries"
                                call = lambda: vb.lookup_top_messages_by_embeddings(qs[:nq], k, thr, allowed)  # noqa: E731
                                coll = lambda: svb.lookup_top_messages_by_embeddings(qs[:nq], k, thr, allowed_s)  # noqa: E731

                                def leg(on: int, reps: int):
                                    geng.set_option("top_messages", on)
                                    return median_ms(call, reps)

                                def shard_lists():
                                    parts = [(g, e, None if allowed is None else allowed.shards[g]) for g, e in enumerate(geng.engines)
                                             if allowed is None or allowed.shards[g] is not None]
                                    t = _native.batch_thresholds(np.float32(thr), nq)
                                    return geng._on_all_parts(parts, _native.batch_queries(qs[:nq], geng.dim), k,
                                                              lambda part, dq, out: part[1].search_top_messages_device(dq, k, t, out_keys=out, dev_rows=part[2])).copy()

                                host_too = not (args.max_host_rows and nq * passing > args.max_host_rows)
                                _, a = leg(1, 1)  # warm-up: workspaces
                                b = leg(0, 1)[1] if host_too else a
                                _, c = median_ms(coll, 1)
                                keys = shard_lists()
                                tn, th, tm, tc_ = [], [], [], []
                                for _ in range(args.rounds):
                                    tn.append(leg(1, args.reps)[0])
                                    if host_too:
                                        th.append(leg(0, args.reps)[0])
                                    tm.append(median_ms(lambda: _native.merge_top_messages_keys(keys), args.reps)[0])
                                    tc_.append(median_ms(coll, args.reps)[0])
                                geng.set_option("top_messages", 1)
                                n, m, cl = float(np.median(tn)), float(np.median(tm)), float(np.median(tc_))
                                identical = same(a, b) and same(a, c)
                                if not host_too:
                                    skipped.append(f"{label}: old route not measured ({nq} x ~{passing} hit objects per call); new {n:.3f} ms, host merge {m:.3f} ms, "
                                                   f"collective {cl:.3f} ms, new == collective: {'yes' if identical else 'NO'}")
                                    print(skipped[-1], flush=True)
                                    continue
                                h = float(np.median(th))
                                spread = (max(th) - min(th)) / h
                                slower = n > h * (1.0 + spread)
                                lines.append(f"| {dtype} | {chunks} | {mask} | {thr:g} | {k} | {nq} | ~{passing} | {n:.3f} | {h:.3f} | {h / n:.2f} | {100 * spread:.1f} % | "
                                             f"{'YES' if slower else 'no'} | {m:.3f} | {cl:.3f} | {'yes' if identical else 'NO'} |")
                                cells.append({"label": label, "new": n, "old": h, "spread": spread, "slower": slower, "same": identical})
                                print(lines[-1], flush=True)
        finally:
            backend.engine.comm_destroy()
        del vb, svb, backend, corpus, geng
        torch.cuda.empty_cache()
    # the device merge alone
    lines += ["", "## The device merge alone (three lists per query, random scores, messages shared between the lists)", "",
              "| n_messages | max_messages | queries | device merge | host merge | bit-identical |", "|---|---|---|---|---|---|"]
    eng = _native.Engine(0)
    rng = np.random.default_rng(5)
    for nm in (int(x) for x in args.merge_messages.split(",")):
        for k in (int(x) for x in args.ks.split(",")):
            for nq in (int(x) for x in args.batches.split(",")):
                host = random_lists(rng, 3, nq, k, nm)
                dev = torch.from_numpy(host).cuda()
                out = torch.empty((nq, k), dtype=torch.int64).pin_memory()

                def device():
                    eng.merge_top_messages_device(dev, nm, out_keys=out)
                    eng.synchronize()
                    return out.numpy().view(np.uint64).copy()

                td, got = median_ms(device, 1)
                td = float(np.median([median_ms(device, args.reps)[0] for _ in range(args.rounds)]))
                th, want = median_ms(lambda: _native.merge_top_messages_keys(host), args.reps)
                lines.append(f"| {nm} | {k} | {nq} | {td:.3f} | {th:.3f} | {'yes' if np.array_equal(got, want) else 'NO'} |")
                print(lines[-1], flush=True)
    eng.close()
    slower = [c for c in cells if c["slower"]]
    lines += ["", "## Reading", "",
              f"- {len(cells)} cells measured against the old route; {len(slower)} slower beyond the spread of its rounds; {sum(c['same'] for c in cells)} of "
              f"{len(cells)} bit-identical between the legs.  They ship behind the switch `top_messages`; no routing rule was fitted.",
              "- Two or more real GPUs remain unmeasured."]
    lines += [f"- SLOWER beyond the spread: {c['label']} -- {c['new']:.3f} ms against {c['old']:.3f} ms ({c['old'] / c['new']:.2f}, spread "
              f"{100 * c['spread']:.1f} %)." for c in slower]
    if skipped:
        lines += ["", "## Old route not measured", ""] + [f"- {s}" for s in skipped]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
