"""Scoped-batch sweep: `fuzzy_lookup_embeddings_scoped` (one row mask per query, ONE submission: tavb_search_scoped_batch) against the loop
it replaces -- one `fuzzy_lookup_embedding_masked` call per query over the same prebuilt `RowMask` handles -- in one process, on one corpus
(default 1M x 1536, fp16 and fp32), for batches of 2 / 8 / 32 queries, scopes of 1 % / 10 % / 50 % of the rows and three overlap patterns:

  identical    every query's scope has the same rows, each in a handle of its own (the SAME handle is no case here: the class hands it to
               `fuzzy_lookup_embeddings_masked`)
  independent  every scope drawn on its own
  disjoint     the rows dealt to floor(1 / share) slots, query q takes slot q mod slots (no two scopes of a pass of eight share a row;
               skipped where eight shares exceed the corpus)

The loop is code this change does not touch, so it is the parent commit's number measured in the same process on the same box.  The two
legs are interleaved: every round times the new call (median of --reps host-synchronous calls) and then the loop; the cell reports the
median over --rounds rounds of each, their ratio (loop / scoped: above 1 the new call wins) and the spread of the loop's rounds
((max - min) / median): a ratio within the spread of 1 is no difference.  Answers are compared bit for bit.  Writes a markdown report:
the table, then a "Reading" section counted from the table's own cells (how many cells, how many at or above the loop, every cell slower
beyond the spread by name, the ratio ranges per overlap pattern and dtype).  Whatever the report file already holds from the line
`KEEP` on -- notes kept by hand, such as the unscoped headline before and after -- is carried over unchanged.

  python tools/scoped_batch_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--k 10] [--reps 5] [--rounds 5] [--out profiles/r20_scoped_batch.md]
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

PATTERNS = ("identical", "independent", "disjoint")
KEEP = "<!-- kept by hand from here on: tools/scoped_batch_sweep.py carries these lines over when it rewrites the file -->"


def reading(cells) -> list[str]:
    """The summary of the table, from its cells: dicts of dtype, pattern, share, nq, scoped, loop, spread, slower, same."""
    at_or_above = [c for c in cells if c["loop"] / c["scoped"] >= 0.995]  # (1.00 as the table prints it)
    slower = [c for c in cells if c["slower"]]
    out = ["", "## Reading", "",
           f"- {len(cells)} cells; {len(at_or_above)} at or above 1.00 (loop / scoped as printed); {len(slower)} slower beyond the spread of the loop's rounds; "
           f"{sum(c['same'] for c in cells)} of {len(cells)} bit-identical to the loop."]
    for c in slower:
        out.append(f"- SLOWER beyond the spread: {c['dtype']}, {c['pattern']} scopes of {100 * c['share']:g} %, {c['nq']} queries -- {c['scoped']:.3f} ms against "
                   f"{c['loop']:.3f} ms ({c['loop'] / c['scoped']:.2f}, spread {100 * c['spread']:.1f} %).")
    for pattern in PATTERNS:
        for dtype in sorted({c["dtype"] for c in cells}):
            for label, pick in (("2 queries", lambda n: n == 2), ("8 and more queries", lambda n: n >= 8)):
                r = [c["loop"] / c["scoped"] for c in cells if c["pattern"] == pattern and c["dtype"] == dtype and pick(c["nq"])]
                if r:
                    out.append(f"- {pattern}, {dtype}, {label}: loop / scoped {min(r):.2f} -- {max(r):.2f} over {len(r)} cells.")
    return out


def kept_tail(path: str) -> list[str]:
    if not os.path.exists(path):
        return []
    old = open(path).read().split("\n")
    return old[old.index(KEEP):] if KEEP in old else []


def median_ms(fn, reps):
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def same(a, b) -> bool:
    """two lists of hit lists equal bit for bit"""
    if [len(x) for x in a] != [len(x) for x in b]:
        return False
    ia = [r.item for q in a for r in q]
    ib = [r.item for q in b for r in q]
    sa = np.array([r.score for q in a for r in q], dtype=np.float32).view(np.uint32)
    sb = np.array([r.score for q in b for r in q], dtype=np.float32).view(np.uint32)
    return ia == ib and np.array_equal(sa, sb)


def scopes_for(vb, pattern: str, share: float, nq: int, rows: int, seed: int):
    """nq RowMask handles, or None where the pattern has no such cell."""
    rng = np.random.default_rng(seed)
    if pattern == "identical":
        m = rng.random(rows) < share
        return [vb.row_mask(m.copy()) for _ in range(nq)]
    if pattern == "independent":
        return [vb.row_mask(rng.random(rows) < share) for _ in range(nq)]
    if 8 * share > 1.0:
        return None
    slots = int(1.0 / share)
    slot = rng.integers(0, slots, rows)
    made = [vb.row_mask(slot == s) for s in range(min(slots, nq))]
    return [made[q % len(made)] for q in range(nq)]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--batches", default="2,8,32")
    ap.add_argument("--shares", default="0.01,0.1,0.5")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_scoped_batch.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    k = args.k
    lines = [
        "# Scoped batches: one row mask per query in one submission, against the loop of single masked calls",
        "",
        "`" + " ".join(["python", "tools/scoped_batch_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)}, max_hits = {k}, min_score = 0, host-synchronous calls, ms.  `scoped` =",
        "`fuzzy_lookup_embeddings_scoped(queries, handles)`; `loop` = `[fuzzy_lookup_embedding_masked(q, h) for q, h in zip(queries, handles)]` over the",
        f"same prebuilt handles.  The legs are interleaved: {args.rounds} rounds of (median of {args.reps} scoped calls, median of {args.reps} loops); the table has the",
        "median over the rounds, `loop / scoped` (above 1: the scoped call is faster) and `spread` = (max - min) / median of the loop's rounds.",
        "`union` = rows in the union of the first pass' scopes.",
        "",
        "| dtype | pattern | share | queries | union | scoped | loop | loop / scoped | spread | slower beyond the spread | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
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
        for pattern in PATTERNS:
            for share in (float(x) for x in args.shares.split(",")):
                for nq in (int(x) for x in args.batches.split(",")):
                    handles = scopes_for(vb, pattern, share, nq, args.rows, int(share * 1000) + nq)
                    if handles is None:
                        continue
                    union = int(np.logical_or.reduce([vb._mask_bools(h) for h in handles[:8]]).sum())
                    scoped = lambda: vb.fuzzy_lookup_embeddings_scoped(qs[:nq], handles, k, 0.0)  # noqa: E731
                    loop = lambda: [vb.fuzzy_lookup_embedding_masked(q, h, k, 0.0) for q, h in zip(qs[:nq], handles)]  # noqa: E731
                    a = scoped()  # warm-up: workspaces
                    assert eng.get_option("masked_route") == 4
                    b = loop()
                    ts, tl = [], []
                    for _ in range(args.rounds):
                        ts.append(median_ms(scoped, args.reps)[0])
                        tl.append(median_ms(loop, args.reps)[0])
                    s, l = float(np.median(ts)), float(np.median(tl))
                    spread = (max(tl) - min(tl)) / l
                    slower = s > l * (1.0 + spread)
                    lines.append(f"| {dtype} | {pattern} | {share:g} | {nq} | {union} | {s:.3f} | {l:.3f} | {l / s:.2f} | {100 * spread:.1f} % | "
                                 f"{'YES' if slower else 'no'} | {'yes' if same(a, b) else 'NO'} |")
                    cells.append({"dtype": dtype, "pattern": pattern, "share": share, "nq": nq, "scoped": s, "loop": l, "spread": spread, "slower": slower,
                                  "same": same(a, b)})
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
