"""Top-k distinct messages under one scope per query: `lookup_top_messages_by_embeddings_scoped` as ONE submission
(tavb_search_top_messages_scoped: per pass of eight queries one scan of the union of their scopes that keeps, per query, one maximum per
message over the rows of that query's own scope; then the exact device top-k over the messages) against the loop over the one-mask call
(`lookup_top_messages_by_embedding(e_i, K, t, scope_i)`, one submission per query) -- in one process, on one corpus (default 1M x 1536,
fp16 and fp32, 3 chunks per message), for scopes of 1 / 10 / 50 % of the rows in three layouts (same-rows: every query its own handle over
the same rows; independent: random rows per query; disjoint: the queries' rows do not overlap, where 8 scopes of that share fit), batches
of 2 / 8 / 32 queries, max_messages 25 / 1000, threshold 0.

Both legs are the same method: the engine option "top_messages_scoped" is 1 for the native call and 0 for the loop.  The legs are
interleaved -- every round times the native call (median of --reps host-synchronous calls) and then the loop -- and the cell reports the
median over --rounds rounds of each, their ratio (loop / native: above 1 the native call wins) and the spread of the loop's rounds
((max - min) / median): a native call slower than the loop by more than that spread is listed.  Answers are compared bit for bit.  Writes a
markdown report; whatever the report file already holds from the line `KEEP` on is carried over unchanged.

  python tools/top_messages_scoped_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--reps 3] [--rounds 3] [--out profiles/r26_top_messages_scoped.md]
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
from tools.scoped_batch_sweep import KEEP, kept_tail, median_ms, same, scopes_for  # noqa: E402,F401
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402

LAYOUTS = {"same-rows": "identical", "independent": "independent", "disjoint": "disjoint"}  # this report's names -> scopes_for's patterns


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--chunks", type=int, default=3)
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--shares", default="0.01,0.1,0.5")
    ap.add_argument("--layouts", default="same-rows,independent,disjoint")
    ap.add_argument("--ks", default="25,1000")
    ap.add_argument("--threshold", type=float, default=0.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_top_messages_scoped.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    props = torch.cuda.get_device_properties(0)
    clock = getattr(props, "clock_rate", None)
    thr = args.threshold
    lines = [
        "# Top-k distinct messages under one scope per query: one submission against the loop over the one-mask call",
        "",
        "`" + " ".join(["python", "tools/top_messages_scoped_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows, {args.chunks} chunks per message, on {torch.cuda.get_device_name(0)} ({props.multi_processor_count} CUs, "
        f"{'clock not reported' if clock is None else f'{clock / 1000:.0f} MHz'}), host-synchronous calls, ms, threshold {thr:g}.  `native` =",
        "`lookup_top_messages_by_embeddings_scoped(queries, scopes, max_messages, threshold)` with the engine option `top_messages_scoped` = 1; `loop` =",
        "the same call with `top_messages_scoped` = 0: one `lookup_top_messages_by_embedding` per query over that query's scope.  The legs are",
        f"interleaved: {args.rounds} rounds of (median of {args.reps} native calls, median of {args.reps} loops); the table has the median over the rounds,",
        "`loop / native` (above 1: the native call is faster) and `spread` = (max - min) / median of the loop's rounds.  `share` = rows of one scope /",
        "rows; `messages` = results of the batch.",
        "",
        "| dtype | layout | share | max_messages | queries | messages | native | loop | loop / native | spread | slower beyond the spread | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells, absent = [], []
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        vb.set_row_messages(np.arange(args.rows, dtype=np.int64) // args.chunks)
        eng = vb.engine
        qs = host_queries(max(int(x) for x in args.batches.split(",")), args.dim, 131)
        for layout in args.layouts.split(","):
            for share in (float(x) for x in args.shares.split(",")):
                for nq in (int(x) for x in args.batches.split(",")):
                    scopes = scopes_for(vb, LAYOUTS[layout], share, nq, args.rows, 77)
                    if scopes is None:
                        absent.append(f"{dtype}, {layout}, share {share:g}, {nq} queries: eight disjoint scopes of that share do not fit the corpus")
                        continue
                    for k in (int(x) for x in args.ks.split(",")):
                        label = f"{dtype}, {layout}, share {share:g}, max_messages {k}, {nq} queries"
                        call = lambda: vb.lookup_top_messages_by_embeddings_scoped(qs[:nq], scopes, k, thr)  # noqa: E731

                        def leg(on: int, reps: int):
                            eng.set_option("top_messages_scoped", on)
                            return median_ms(call, reps)

                        _, a = leg(1, 1)  # warm-up: workspaces
                        route = eng.get_option("masked_route")
                        _, b = leg(0, 1)
                        tn, tl = [], []
                        for _ in range(args.rounds):
                            tn.append(leg(1, args.reps)[0])
                            tl.append(leg(0, args.reps)[0])
                        eng.set_option("top_messages_scoped", 1)
                        n, lo = float(np.median(tn)), float(np.median(tl))
                        spread = (max(tl) - min(tl)) / lo
                        slower = n > lo * (1.0 + spread)
                        ok = same(a, b) and route == 9
                        lines.append(f"| {dtype} | {layout} | {share:g} | {k} | {nq} | {sum(len(x) for x in a)} | {n:.3f} | {lo:.3f} | {lo / n:.2f} | "
                                     f"{100 * spread:.1f} % | {'YES' if slower else 'no'} | {'yes' if ok else 'NO'} |")
                        cells.append({"label": label, "dtype": dtype, "layout": layout, "share": share, "native": n, "loop": lo, "spread": spread,
                                      "slower": slower, "same": ok})
                        print(lines[-1], flush=True)
                    del scopes
        del vb, corpus, eng
        torch.cuda.empty_cache()
    slower = [c for c in cells if c["slower"]]
    lines += ["", "## Reading", "",
              f"- {len(cells)} cells measured; {len(slower)} slower beyond the spread of the loop's rounds; {sum(c['same'] for c in cells)} of {len(cells)} "
              "bit-identical between the legs (and served by the native route, `masked_route` 9)."]
    for layout in args.layouts.split(","):
        for share in (float(x) for x in args.shares.split(",")):
            r = [c["loop"] / c["native"] for c in cells if c["layout"] == layout and c["share"] == share]
            if r:
                lines.append(f"- {layout}, share {share:g}: loop / native {min(r):.2f} -- {max(r):.2f} over {len(r)} cells.")
    lines += [f"- SLOWER beyond the spread: {c['label']} -- {c['native']:.3f} ms against {c['loop']:.3f} ms ({c['loop'] / c['native']:.2f}, spread "
              f"{100 * c['spread']:.1f} %).  Ships; `top_messages_scoped` = 0 is the switch." for c in slower]
    if absent:
        lines += ["", "## No such cell", ""] + [f"- {s}" for s in absent]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
