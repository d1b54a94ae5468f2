"""Scope algebra on the device against the host route it replaces: one process, one corpus (default 1M x 1536 fp16 rows, 3 chunk rows per
message), scopes of 1 / 10 / 50 % of the messages given by 1, 2 and 4 selectors (each a range of message ordinals; their intersection is
the scope), then ONE scoped message query (`lookup_messages_by_embeddings_masked`, max_matches 10).

  device    `range_mask(collections, of="messages")` (tavb_mask_from_ranges + the row list), then the query
  host      every selector enumerated to its ordinals, np.intersect1d over them, `message_mask` (tavb_mask_from_messages + tavb_mask_expand),
            then the query -- unchanged code: the parent commit's figure of the cell; `host2` = the same leg again, `spread` = slowest -
            fastest of the two legs' timed calls
  build     the two legs without the query: `dev build` / `host build`

and `a & b` alone on two resident handles (tavb_mask_combine + the row list) against `row_mask(A & B)` of a fresh host bool array.  Legs
are interleaved (one call of each per round, `--reps` rounds after a warm-up round), medians of host-synchronous calls in ms.  `equal` =
both legs return the same messages and score bits.

  python tools/mask_algebra_sweep.py [--rows 1000000] [--reps 9] [--out profiles/r17_mask_algebra.md]
"""

from __future__ import annotations

import argparse
import os
import sys
from functools import reduce

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import host_queries, make_device_corpus  # noqa: E402
from tests.fakes import NullModel  # noqa: E402
from tools.masked_tile_sweep import interleaved  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402


def selectors(n_messages: int, share: float, n: int) -> list[list[tuple[int, int]]]:
    """n selectors, one range of message ordinals each, whose intersection is `share` of the messages: the window, widened on alternate sides."""
    width = int(n_messages * share)
    lo = int(0.3 * n_messages) + 7
    slack = max((n_messages - lo - width) // 8, 1)
    return [[(lo - (i % 2) * (i + 1) * min(slack, lo // 8), lo + width + ((i + 1) % 2) * (i + 1) * slack)] for i in range(n)] if n > 1 else [[(lo, lo + width)]]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_mask_algebra.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype="fp16")
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, "fp16")
    eng0.close()
    vb.adopt_device_corpus(corpus)
    n_messages = (args.rows + 2) // 3
    vb.set_row_messages(np.arange(args.rows, dtype=np.int64) // 3)
    q = host_queries(1, args.dim, 131)
    lines = [
        "# Scope algebra on the device against host enumeration + np.intersect1d + message_mask",
        "",
        "`" + " ".join(["python", "tools/mask_algebra_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} fp16 rows, {n_messages} messages, on {torch.cuda.get_device_name(0)}; one scoped message query (max_matches 10, threshold 0);",
        f"legs interleaved, medians of {args.reps} host-synchronous calls after a warm-up round, ms.  Legs and columns: the tool's docstring.",
        "",
        "| scope | selectors | rows allowed | device | host | host2 | spread | device / host | dev build | host build | equal |",
        "|---|---|---|---|---|---|---|---|---|---|---|",
    ]

    def bits(lists):
        return [[(h.item, int(np.float32(h.score).view(np.uint32))) for h in one] for one in lists]

    for share in (0.01, 0.1, 0.5):
        for n in (1, 2, 4):
            cols = selectors(n_messages, share, n)

            def host_mask():
                ords = reduce(np.intersect1d, [np.concatenate([np.arange(max(s, 0), min(e, n_messages), dtype=np.int64) for s, e in c]) for c in cols])
                return vb.message_mask(ords)

            def dev_mask():
                return vb.range_mask(cols, of="messages")

            def query(build):
                return lambda: vb.lookup_messages_by_embeddings_masked(q, build(), 10, 0.0)

            med, out, every = interleaved({"device": query(dev_mask), "host": query(host_mask), "host2": query(host_mask), "dev build": dev_mask,
                                           "host build": host_mask}, args.reps)
            both = every["host"] + every["host2"]
            lines.append(f"| {share:.0%} | {n} | {out['dev build'].count} | {med['device']:.3f} | {med['host']:.3f} | {med['host2']:.3f} | {max(both) - min(both):.3f} | "
                         f"{med['device'] / med['host']:.2f} | {med['dev build']:.3f} | {med['host build']:.3f} | "
                         f"{bits(out['device']) == bits(out['host']) and out['dev build'].count == out['host build'].count} |")
            print(lines[-1], flush=True)

    lines += ["", "## `a & b` on resident handles against `row_mask` of a fresh host bool array", "",
              "| density of a, b | rows allowed | a & b (device) | row_mask(A & B) | row_mask again | spread | device / host | equal |", "|---|---|---|---|---|---|---|---|"]
    for dens in (0.1, 0.5, 0.9):
        rng = np.random.default_rng(int(dens * 100))
        A, B = rng.random(args.rows) < dens, rng.random(args.rows) < dens
        a, b = vb.row_mask(A), vb.row_mask(B)
        med, out, every = interleaved({"device": lambda: a & b, "host": lambda: vb.row_mask(A & B), "host2": lambda: vb.row_mask(A & B)}, args.reps)
        both = every["host"] + every["host2"]
        same = bool(torch.equal(out["device"].dev_rows, out["host"].dev_rows) and torch.equal(out["device"].dev_bits, out["host"].dev_bits))
        lines.append(f"| {dens} | {out['device'].count} | {med['device']:.3f} | {med['host']:.3f} | {med['host2']:.3f} | {max(both) - min(both):.3f} | "
                     f"{med['device'] / med['host']:.2f} | {same and out['device'].span == out['host'].span} |")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
