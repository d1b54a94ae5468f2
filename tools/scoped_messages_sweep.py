"""Scoped message lookups: a scope of message ordinals searched as a device-built row mask (`VectorBase.message_mask`,
`lookup_messages_by_embeddings_masked`) against the host route it replaces, in one process on one corpus (default 1M x 1536 fp16, about 3
chunks per message) at scopes of 1, 10 and 50 % of the messages.

(a) a FRESH scope, one query
  parent    np.isin over the host map -> np.flatnonzero -> the Python row list -> lookup_messages_in_subset_by_embedding (its conversion,
            range check and upload of the list, then the lookup): what a caller does today
  parent2   the same leg again, interleaved
  mask      message_mask(scope) alone (ordinals up, mask and row list built on the device)
  new       message_mask(scope) + lookup_messages_by_embedding_masked
(b) 1, 8, 32 and 256 lookups over a scope that is already expanded
  parent    that many sequential lookup_messages_in_subset_by_embedding calls over the SAME row list (converted and uploaded by every call)
  parent2   the same leg again, interleaved
  new       ONE lookup_messages_by_embeddings_masked call over the RowMask, at the default options (`route` = what it took)

Legs are interleaved (one call of each per round, `--reps` rounds after a warm-up round), medians of host-synchronous calls in ms.  `spread`
= slowest - fastest of the two parent legs' timed calls; every cell is given as new / parent next to spread / parent.  `equal` = the new
leg's messages, float32 scores and counts are the parent's, bit for bit.  Writes a markdown report (default profiles/r16_scoped_messages.md).

  python tools/scoped_messages_sweep.py [--rows 1000000] [--dim 1536] [--dtype fp16] [--scopes 0.01,0.1,0.5] [--batches 1,8,32,256] [--k 10] [--reps 3] [--out ...]
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


def interleaved(legs: dict, reps: int) -> tuple[dict, dict, dict]:
    """{name: fn} -> ({name: median ms}, {name: last result}, {name: every timed call, ms}); one call of every leg per round, the first round not timed"""
    times = {name: [] for name in legs}
    out = {}
    for rnd in range(reps + 1):
        for name, fn in legs.items():
            t0 = time.perf_counter()
            out[name] = fn()
            if rnd:
                times[name].append(time.perf_counter() - t0)
    return {name: float(np.median(ts)) * 1e3 for name, ts in times.items()}, out, {name: [t * 1e3 for t in ts] for name, ts in times.items()}


def bits(lists) -> list:
    return [[(h.item, int(np.float32(h.score).view(np.uint32))) for h in hits] for hits in lists]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--scopes", default="0.01,0.1,0.5")
    ap.add_argument("--batches", default="1,8,32,256")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_scoped_messages.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    batches = [int(x) for x in args.batches.split(",")]
    k = args.k
    rng = np.random.default_rng(1601)
    row_messages = np.repeat(np.arange(args.rows, dtype=np.int64), rng.integers(1, 6, size=args.rows))[: args.rows]  # 1 to 5 chunks per message, contiguous
    n_messages = int(row_messages.max()) + 1

    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=args.dtype)
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, args.dtype)
    eng0.close()
    vb.adopt_device_corpus(corpus)
    vb.set_row_messages(row_messages)
    eng = vb.engine
    qs = host_queries(max(batches), args.dim, 131)

    lines = [
        "# Scoped message lookups: a device-built mask against the host row list",
        "",
        "`" + " ".join(["python", "tools/scoped_messages_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} {args.dtype} rows, {n_messages} messages of 1 to 5 chunks, on {torch.cuda.get_device_name(0)}; max_matches = {k}, threshold 0; legs",
        f"interleaved, medians of {args.reps} host-synchronous calls after a warm-up round, ms.  `parent` is the route a caller takes without this",
        "feature; `parent2` the same leg a second time; `spread` = slowest - fastest of the two legs' timed calls.  `new / parent` below 1 is a gain;",
        "a cell is slower than the route it replaces when `new / parent` exceeds 1 + `spread / parent`.",
        "",
        "## (a) a fresh scope, one query",
        "",
        "| scope | messages | rows allowed | parent | parent2 | spread | mask alone | new (mask + lookup) | new / parent | spread / parent | equal |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    table_b = [
        "## (b) lookups over an expanded scope",
        "",
        "| scope | rows allowed | queries | parent (sequential) | parent2 | spread | new (one call) | route | new / parent | spread / parent | equal |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for share in (float(x) for x in args.scopes.split(",")):
        scope = np.sort(np.random.default_rng(int(share * 1000)).choice(n_messages, size=int(share * n_messages), replace=False)).astype(np.int64)
        q0 = qs[0]

        def parent_fresh():
            rows = np.flatnonzero(np.isin(row_messages, scope) & (row_messages >= 0)).tolist()
            return [vb.lookup_messages_in_subset_by_embedding(q0, rows, k, 0.0)]

        def new_fresh():
            return [vb.lookup_messages_by_embedding_masked(q0, vb.message_mask(scope), k, 0.0)]

        ms, out, calls = interleaved({"parent": parent_fresh, "mask": lambda: vb.message_mask(scope), "parent2": parent_fresh, "new": new_fresh}, args.reps)
        both = calls["parent"] + calls["parent2"]
        spread = max(both) - min(both)
        handle = out["mask"]
        row = [f"{share:g}", str(len(scope)), str(handle.count), f"{ms['parent']:.3f}", f"{ms['parent2']:.3f}", f"{spread:.3f}", f"{ms['mask']:.3f}", f"{ms['new']:.3f}",
               f"{ms['new'] / ms['parent']:.3f}", f"{spread / ms['parent']:.3f}", "yes" if bits(out["new"]) == bits(out["parent"]) else "NO"]
        lines.append("| " + " | ".join(row) + " |")
        print(lines[-1], flush=True)

        rows_list = handle.flat().tolist()
        for nq in batches:
            q = qs[:nq]
            routes = {}

            def parent_seq():
                return [vb.lookup_messages_in_subset_by_embedding(e, rows_list, k, 0.0) for e in q]

            def new_batch():
                r = vb.lookup_messages_by_embeddings_masked(q, handle, k, 0.0)
                routes["new"] = eng.get_option("masked_route")
                return r

            ms, out, calls = interleaved({"parent": parent_seq, "new": new_batch, "parent2": parent_seq}, args.reps)
            both = calls["parent"] + calls["parent2"]
            spread = max(both) - min(both)
            row = [f"{share:g}", str(handle.count), str(nq), f"{ms['parent']:.3f}", f"{ms['parent2']:.3f}", f"{spread:.3f}", f"{ms['new']:.3f}", str(routes["new"]),
                   f"{ms['new'] / ms['parent']:.4f}", f"{spread / ms['parent']:.4f}", "yes" if bits(out["new"]) == bits(out["parent"]) else "NO"]
            table_b.append("| " + " | ".join(row) + " |")
            print(table_b[-1], flush=True)
    text = "\n".join(lines + [""] + table_b) + "\n"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
