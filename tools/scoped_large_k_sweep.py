"""Scoped batches beyond max_hits 256: `fuzzy_lookup_embeddings_scoped` as ONE submission (tavb_search_scoped_topk for max_hits 257 ..
16384, tavb_search_scoped_sorted for max_hits 0 and beyond) against the loop it replaces -- one `fuzzy_lookup_embedding_masked` call per
query -- in one process, on one corpus (default 1M x 1536, fp16 and fp32), for batches of 2 / 8 / 32 queries, scopes of 1 % / 10 % / 50 %
of the rows in the three overlap patterns of tools/scoped_batch_sweep.py (identical, independent, disjoint), and two lookups:

  max_hits 1000 at min_score 0                      the large-k route
  max_hits 0 at a min_score that leaves about 1 %   the sorted route: every survivor of the scope
  of a scope (the score of the query-0 hit at rank rows / 100 over the whole corpus)

Both legs are the same method on the same handles: the engine option "scope_large_k" is 1 for the new call and 0 for the loop, which is
then the code of before this route.  The legs are interleaved -- every round times the new call (median of --reps host-synchronous calls)
and then the loop -- and the cell reports the median over --rounds rounds of each, their ratio (loop / scoped: above 1 the new call wins)
and the spread of the loop's rounds ((max - min) / median): a ratio within the spread of 1 is no difference.  Answers are compared bit for
bit.  Writes a markdown report: the device and its clock, the table, then the "Reading" section of tools/scoped_batch_sweep.py counted
from the table's own cells, per lookup.  Whatever the report file already holds from the line `KEEP` on is carried over unchanged.

  python tools/scoped_large_k_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--reps 5] [--rounds 5] [--out profiles/r23_scoped_large_k.md]
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
from tools.scoped_batch_sweep import KEEP, PATTERNS, kept_tail, median_ms, reading, same, scopes_for  # noqa: E402,F401
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--shares", default="0.01,0.1,0.5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_scoped_large_k.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    props = torch.cuda.get_device_properties(0)
    clock = getattr(props, "clock_rate", None)
    lines = [
        "# Scoped batches at max_hits 1000 and 0: one submission against the loop of single masked calls",
        "",
        "`" + " ".join(["python", "tools/scoped_large_k_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)} ({props.multi_processor_count} CUs, "
        f"{'clock not reported' if clock is None else f'{clock / 1000:.0f} MHz'}), host-synchronous calls, ms.  `scoped` =",
        "`fuzzy_lookup_embeddings_scoped(queries, handles, max_hits, min_score)` with the engine option `scope_large_k` = 1; `loop` = the same call",
        f"with `scope_large_k` = 0, which loops over `fuzzy_lookup_embedding_masked`.  The legs are interleaved: {args.rounds} rounds of (median of {args.reps}",
        f"scoped calls, median of {args.reps} loops); the table has the median over the rounds, `loop / scoped` (above 1: the scoped call is faster) and",
        "`spread` = (max - min) / median of the loop's rounds.  `union` = rows in the union of the first pass' scopes; `hits` = results of the batch.",
        "",
        "| dtype | max_hits | min_score | pattern | share | queries | union | hits | scoped | loop | loop / scoped | spread | slower beyond the spread | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells = []
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        qs = host_queries(32, args.dim, 131)
        one_pct = float(vb.fuzzy_lookup_embedding(qs[0], max_hits=max(args.rows // 100, 1), min_score=0.0)[-1].score)
        for max_hits, thr in ((1000, 0.0), (0, one_pct)):
            for pattern in PATTERNS:
                for share in (float(x) for x in args.shares.split(",")):
                    for nq in (int(x) for x in args.batches.split(",")):
                        handles = scopes_for(vb, pattern, share, nq, args.rows, int(share * 1000) + nq)
                        if handles is None:
                            continue
                        union = int(np.logical_or.reduce([vb._mask_bools(h) for h in handles[:8]]).sum())
                        call = lambda: vb.fuzzy_lookup_embeddings_scoped(qs[:nq], handles, max_hits, thr)  # noqa: E731

                        def leg(on: int, reps: int):
                            eng.set_option("scope_large_k", on)
                            return median_ms(call, reps)

                        _, a = leg(1, 1)  # warm-up: workspaces
                        assert eng.get_option("masked_route") == (7 if max_hits else 8)
                        _, b = leg(0, 1)
                        ts, tl = [], []
                        for _ in range(args.rounds):
                            ts.append(leg(1, args.reps)[0])
                            tl.append(leg(0, args.reps)[0])
                        eng.set_option("scope_large_k", 1)
                        s, l = float(np.median(ts)), float(np.median(tl))
                        spread = (max(tl) - min(tl)) / l
                        slower = s > l * (1.0 + spread)
                        lines.append(f"| {dtype} | {max_hits} | {thr:.4f} | {pattern} | {share:g} | {nq} | {union} | {sum(len(x) for x in a)} | {s:.3f} | {l:.3f} | "
                                     f"{l / s:.2f} | {100 * spread:.1f} % | {'YES' if slower else 'no'} | {'yes' if same(a, b) else 'NO'} |")
                        cells.append({"dtype": f"{dtype} max_hits {max_hits}", "pattern": pattern, "share": share, "nq": nq, "scoped": s, "loop": l,
                                      "spread": spread, "slower": slower, "same": same(a, b)})
                        print(lines[-1], flush=True)
                        del handles
        del vb, corpus, eng
        torch.cuda.empty_cache()
    lines += reading(cells)
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
