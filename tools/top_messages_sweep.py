"""Top-k distinct messages: `lookup_top_messages_by_embeddings` as ONE submission (tavb_search_top_messages: a per-message maximum kept on
the device during the corpus pass, then the exact device top-k over the messages) against the only way to the same answer before it -- the
all-survivor lookup (`fuzzy_lookup_embeddings` / `_masked` at max_hits = 0: the score pass that writes 4 bytes per row and query, the
device sort of every survivor, the hit objects built on the host) and a collapse on the host -- in one process, on one corpus (default
1M x 1536, fp16 and fp32), for 3 and 8 chunks per message, batches of 1 / 8 / 32 queries, max_messages 25 / 1000, thresholds 0 and 0.7,
unmasked and under a 10 % random row mask.

Both legs are the same method: the engine option "top_messages" is 1 for the native call and 0 for the host collapse.  The legs are
interleaved -- every round times the native call (median of --reps host-synchronous calls) and then the host leg -- and the cell reports
the median over --rounds rounds of each, their ratio (host / native: above 1 the native call wins) and the spread of the host leg's rounds
((max - min) / median): a native call slower than the host leg by more than that spread is listed.  Answers are compared bit for bit.
`--max-host-rows` skips the cells whose host leg would build more than that many hit objects per call (queries x passing rows; 0 = no
limit): they are listed as not measured.  Writes a markdown report; whatever the report file already holds from the line `KEEP` on is
carried over unchanged.

  python tools/top_messages_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--reps 3] [--rounds 3] [--out profiles/r25_top_messages.md]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--chunks", default="3,8")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--ks", default="25,1000")
    ap.add_argument("--thresholds", default="0,0.7")
    ap.add_argument("--masks", default="none,10%")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-host-rows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_top_messages.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    props = torch.cuda.get_device_properties(0)
    clock = getattr(props, "clock_rate", None)
    lines = [
        "# Top-k distinct messages: one submission against the all-survivor lookup and a host collapse",
        "",
        "`" + " ".join(["python", "tools/top_messages_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)} ({props.multi_processor_count} CUs, "
        f"{'clock not reported' if clock is None else f'{clock / 1000:.0f} MHz'}), host-synchronous calls, ms.  `native` =",
        "`lookup_top_messages_by_embeddings(queries, max_messages, threshold, allowed)` with the engine option `top_messages` = 1; `host` = the same",
        f"call with `top_messages` = 0: every survivor sorted on the device, collapsed on the host.  The legs are interleaved: {args.rounds} rounds of",
        f"(median of {args.reps} native calls, median of {args.reps} host calls); the table has the median over the rounds, `host / native` (above 1: the",
        "native call is faster) and `spread` = (max - min) / median of the host leg's rounds.  `passing` = rows of query 0 that pass the threshold",
        "inside the allowed set; `messages` = results of the batch.",
        "",
        "| dtype | chunks / message | mask | threshold | max_messages | queries | passing | messages | native | host | host / native | spread | slower beyond the spread | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells, skipped = [], []
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        qs = host_queries(32, args.dim, 131)
        handles = {"none": None, "10%": vb.row_mask(np.random.default_rng(77).random(args.rows) < 0.1)}
        for chunks in (int(x) for x in args.chunks.split(",")):
            vb.set_row_messages(np.arange(args.rows, dtype=np.int64) // chunks)
            for mask in args.masks.split(","):
                allowed = handles[mask]
                for thr in (float(x) for x in args.thresholds.split(",")):
                    eng.set_option("top_messages", 1)
                    passing = len(vb.fuzzy_lookup_embedding(qs[0], 0, thr) if allowed is None else vb.fuzzy_lookup_embedding_masked(qs[0], allowed, 0, thr))
                    for k in (int(x) for x in args.ks.split(",")):
                        for nq in (int(x) for x in args.batches.split(",")):
                            label = f"{dtype}, {chunks} chunks, mask {mask}, threshold {thr:g}, max_messages {k}, {nq} queries"
                            call = lambda: vb.lookup_top_messages_by_embeddings(qs[:nq], k, thr, allowed)  # noqa: E731

                            def leg(on: int, reps: int):
                                eng.set_option("top_messages", on)
                                return median_ms(call, reps)

                            if args.max_host_rows and nq * passing > args.max_host_rows:
                                t, a = leg(1, args.reps)
                                skipped.append(f"{label}: host leg not measured ({nq} x {passing} hit objects per call); native {t:.3f} ms, {sum(len(x) for x in a)} messages")
                                print(skipped[-1], flush=True)
                                continue
                            _, a = leg(1, 1)  # warm-up: workspaces
                            _, b = leg(0, 1)
                            tn, th = [], []
                            for _ in range(args.rounds):
                                tn.append(leg(1, args.reps)[0])
                                th.append(leg(0, args.reps)[0])
                            eng.set_option("top_messages", 1)
                            n, h = float(np.median(tn)), float(np.median(th))
                            spread = (max(th) - min(th)) / h
                            slower = n > h * (1.0 + spread)
                            lines.append(f"| {dtype} | {chunks} | {mask} | {thr:g} | {k} | {nq} | {passing} | {sum(len(x) for x in a)} | {n:.3f} | {h:.3f} | "
                                         f"{h / n:.2f} | {100 * spread:.1f} % | {'YES' if slower else 'no'} | {'yes' if same(a, b) else 'NO'} |")
                            cells.append({"label": label, "native": n, "host": h, "spread": spread, "slower": slower, "same": same(a, b)})
                            print(lines[-1], flush=True)
        del vb, corpus, eng, handles
        torch.cuda.empty_cache()
    slower = [c for c in cells if c["slower"]]
    lines += ["", "## Reading", "",
              f"- {len(cells)} cells measured; {len(slower)} slower beyond the spread of the host leg's rounds; {sum(c['same'] for c in cells)} of {len(cells)} "
              "bit-identical between the legs."]
    lines += [f"- SLOWER beyond the spread: {c['label']} -- {c['native']:.3f} ms against {c['host']:.3f} ms ({c['host'] / c['native']:.2f}, spread "
              f"{100 * c['spread']:.1f} %)." for c in slower]
    if skipped:
        lines += ["", "## Not measured", ""] + [f"- {s}" for s in skipped]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
