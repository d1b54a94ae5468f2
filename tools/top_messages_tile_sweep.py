"""Top-k distinct messages on the 32/64-query MFMA tile: `lookup_top_messages_by_embeddings` with the engine option "top_messages_tile" = 2
(tavb_search_top_messages_tile: one corpus pass per 64 queries, one atomic max per admitted (row, query) pair) against the same call with
the option at 0 (tavb_search_top_messages: one pass of the row scan per eight queries) -- in one process, on one corpus (default
1M x 1536, fp16 and fp32), for 3 and 8 chunks per message, batches of 8 / 16 / 32 / 64 / 256 queries, max_messages 25 / 1000, threshold 0
(every (row, query) pair does its atomic: the worst case) and a threshold about 1 % of the rows pass (`--tail`: the quantile of query 0's
scores), unmasked and under random row masks of 10 %, 50 % and 100 %.

The legs are interleaved -- every round times the tile leg (median of --reps host-synchronous calls) and then the scan leg -- and the cell
reports the median over --rounds rounds of each, their ratio (scan / tile: above 1 the tile wins) and the spread of the scan leg's rounds
((max - min) / median): a tile leg slower than the scan leg by more than that spread is listed.  The two legs' scores differ in the last
bits (the tile's own summation order), so the answers are compared as sets of message ordinals per query, and the largest score
difference over the common messages is reported.  Writes a markdown report; whatever the report file already holds from the line `KEEP`
on is carried over unchanged.

  python tools/top_messages_tile_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--reps 3] [--rounds 3] [--out profiles/r27_top_messages_tile.md]
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
from tools.scoped_batch_sweep import KEEP, kept_tail, median_ms  # noqa: E402,F401
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402


def agreement(a, b):
    """(queries whose message sets differ, largest |score difference| over the messages both legs return)."""
    differ, worst = 0, 0.0
    for x, y in zip(a, b):
        sx, sy = {h.item: h.score for h in x}, {h.item: h.score for h in y}
        differ += set(sx) != set(sy)
        worst = max([worst] + [abs(sx[m] - sy[m]) for m in sx.keys() & sy.keys()])
    return differ, worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--chunks", default="3,8")
    ap.add_argument("--batches", default="8,16,32,64,256")
    ap.add_argument("--ks", default="25,1000")
    ap.add_argument("--tail", type=float, default=0.01, help="share of the rows the second threshold lets pass for query 0")
    ap.add_argument("--masks", default="none,10%,50%,100%")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r27_top_messages_tile.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    props = torch.cuda.get_device_properties(0)
    clock = getattr(props, "clock_rate", None)
    lines = [
        "# Top-k distinct messages on the 32/64-query tile against the row scan",
        "",
        "`" + " ".join(["python", "tools/top_messages_tile_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)} ({props.multi_processor_count} CUs, "
        f"{'clock not reported' if clock is None else f'{clock / 1000:.0f} MHz'}), host-synchronous calls, ms.  `tile` =",
        "`lookup_top_messages_by_embeddings(queries, max_messages, threshold, allowed)` with the engine option `top_messages_tile` = 2; `scan` = the",
        f"same call with the option at 0.  The legs are interleaved: {args.rounds} rounds of (median of {args.reps} tile calls, median of {args.reps} scan calls);",
        "the table has the median over the rounds, `scan / tile` (above 1: the tile is faster) and `spread` = (max - min) / median of the scan leg's",
        "rounds.  `passing` = rows of query 0 that pass the threshold inside the allowed set; `sets differ` = queries whose two answers name different",
        "messages (near-ties at rank K); `max score diff` over the messages both answers hold.",
        "",
        "| dtype | chunks / message | mask | threshold | max_messages | queries | passing | tile | scan | scan / tile | spread | slower beyond the spread | sets differ | max score diff |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells = []
    most = max(int(x) for x in args.batches.split(","))
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        qs = host_queries(most, args.dim, 131)
        rng = np.random.default_rng(77)
        handles = {"none": None}
        for name in args.masks.split(","):
            if name != "none":
                handles[name] = vb.row_mask(rng.random(args.rows) < float(name.rstrip("%")) / 100.0 if name != "100%" else np.ones(args.rows, dtype=bool))
        all_scores = np.asarray([h.score for h in vb.fuzzy_lookup_embedding(qs[0], 0, 0.0)], dtype=np.float64)
        tail_thr = float(np.quantile(all_scores, 1.0 - args.tail))
        del all_scores
        for chunks in (int(x) for x in args.chunks.split(",")):
            vb.set_row_messages(np.arange(args.rows, dtype=np.int64) // chunks)
            for mask in args.masks.split(","):
                allowed = handles[mask]
                for thr in (0.0, tail_thr):
                    passing = len(vb.fuzzy_lookup_embedding(qs[0], 0, thr) if allowed is None else vb.fuzzy_lookup_embedding_masked(qs[0], allowed, 0, thr))
                    for k in (int(x) for x in args.ks.split(",")):
                        for nq in (int(x) for x in args.batches.split(",")):
                            label = f"{dtype}, {chunks} chunks, mask {mask}, threshold {thr:.4g}, max_messages {k}, {nq} queries"
                            call = lambda: vb.lookup_top_messages_by_embeddings(qs[:nq], k, thr, allowed)  # noqa: E731

                            def leg(on: int, reps: int):
                                eng.set_option("top_messages_tile", on)
                                return median_ms(call, reps)

                            _, a = leg(2, 1)  # warm-up: workspaces
                            assert eng.get_option("masked_route") == 10 and eng.get_option("last_tier") == 5
                            _, b = leg(0, 1)
                            tt, ts = [], []
                            for _ in range(args.rounds):
                                tt.append(leg(2, args.reps)[0])
                                ts.append(leg(0, args.reps)[0])
                            eng.set_option("top_messages_tile", 0)
                            t, s = float(np.median(tt)), float(np.median(ts))
                            spread = (max(ts) - min(ts)) / s
                            slower = t > s * (1.0 + spread)
                            differ, worst = agreement(a, b)
                            lines.append(f"| {dtype} | {chunks} | {mask} | {thr:.4g} | {k} | {nq} | {passing} | {t:.3f} | {s:.3f} | {s / t:.2f} | "
                                         f"{100 * spread:.1f} % | {'YES' if slower else 'no'} | {differ} | {worst:.1e} |")
                            cells.append({"label": label, "tile": t, "scan": s, "spread": spread, "slower": slower})
                            print(lines[-1], flush=True)
        del vb, corpus, eng, handles
        torch.cuda.empty_cache()
    slower = [c for c in cells if c["slower"]]
    lines += ["", "## Reading", "", f"- {len(cells)} cells measured; {len(slower)} slower beyond the spread of the scan leg's rounds."]
    lines += [f"- SLOWER beyond the spread: {c['label']} -- {c['tile']:.3f} ms against {c['scan']:.3f} ms ({c['scan'] / c['tile']:.2f}, spread "
              f"{100 * c['spread']:.1f} %)." for c in slower]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
