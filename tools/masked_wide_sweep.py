"""Masked batches of 128+ queries on an fp16 corpus: the row list (eight queries per pass), the 32/64-query tile and the 128/256-query filter tile
+ rescoring (tavb_search_masked_wide), each forced, next to what the options picked before the wide route existed and what they pick now --
one process, one corpus (default 1M x 1536 fp16), masks of 10 % and 50 % random, a contiguous 50 % range and 100 %.

  rowlist   mask_wide = 0, mask_tile = 0
  tile      mask_wide = 0, mask_tile = 2
  wide      mask_wide = 2
  parent    mask_wide = 0, mask_tile = 1: the defaults as they were before this route -- the parent's time of the cell; `parent2` = the same leg again,
            `spread` = slowest - fastest of the two legs' timed calls
  default   mask_wide = 1, mask_tile = 1 (the shipped options); `route` = what it took (1 = row list, 2 = 32/64-query tile, 3 = wide)
  unmasked  (100 % only) fuzzy_lookup_embeddings of the same batch, in the same process: what the bit test costs

Legs are interleaved (one call of each per round, `--reps` rounds after a warm-up round), medians of host-synchronous calls in ms, all through
`as_arrays=True`.  `equal` = the wide route's ordinals, score bits and counts equal the row list's.  Writes profiles/r15_masked_wide.md.

  python tools/masked_wide_sweep.py [--rows 1000000] [--batches 128,256,1024] [--k 10] [--reps 5] [--out ...]
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
from tools.masked_tile_sweep import interleaved  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--batches", default="128,256,1024")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_masked_wide.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    batches = [int(x) for x in args.batches.split(",")]
    k = args.k
    lines = [
        "# Masked batches of 128+ queries: row list, 32/64-query tile, 128/256-query filter tile + rescoring",
        "",
        "`" + " ".join(["python", "tools/masked_wide_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} fp16 rows on {torch.cuda.get_device_name(0)}, max_hits = {k}, min_score = 0; legs interleaved, medians of {args.reps} host-synchronous",
        "calls after a warm-up round, ms.  Legs and columns: the tool's docstring.",
        "",
        "| mask | rows allowed | span | queries | rowlist | tile | wide | parent | parent2 | spread | default | route | tile / wide | default - parent | unmasked | wide / unmasked | equal |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype="fp16")
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, "fp16")
    eng0.close()
    vb.adopt_device_corpus(corpus)
    eng = vb.engine
    qs = host_queries(max(batches), args.dim, 131)
    for name, dens in (("random 0.1", 0.1), ("random 0.5", 0.5), ("contiguous 0.5", 0.5), ("all", 1.0)):
        if name.startswith("random"):
            mask = np.random.default_rng(int(dens * 1000)).random(args.rows) < dens
        elif name.startswith("contiguous"):  # unaligned ends
            lo = int(0.3 * args.rows) + 7
            mask = np.zeros(args.rows, dtype=bool)
            mask[lo: lo + int(dens * args.rows)] = True
        else:
            mask = np.ones(args.rows, dtype=bool)
        handle = vb.row_mask(mask)
        span = handle.span[1] + 1 - handle.span[0] // 256 * 256
        for nq in batches:
            q = qs[:nq]
            routes = {}

            def leg(wide, tile, tag=None):
                def run():
                    eng.set_option("mask_wide", wide)
                    eng.set_option("mask_tile", tile)
                    r = vb.fuzzy_lookup_embeddings_masked(q, handle, k, 0.0, as_arrays=True)
                    if tag:
                        routes[tag] = eng.get_option("masked_route")
                    return r
                return run

            legs = {"rowlist": leg(0, 0), "tile": leg(0, 2), "wide": leg(2, 0, "wide"), "parent": leg(0, 1), "default": leg(1, 1, "default"), "parent2": leg(0, 1)}
            if dens >= 1:
                legs["unmasked"] = lambda: vb.fuzzy_lookup_embeddings(q, k, 0.0, as_arrays=True)
            ms, out, calls = interleaved(legs, args.reps)
            eng.set_option("mask_wide", 1)
            eng.set_option("mask_tile", 1)
            assert routes["wide"] == 3
            both = calls["parent"] + calls["parent2"]
            (o, s, c), (o2, s2, c2) = out["wide"], out["rowlist"]
            live = np.arange(o.shape[1])[None, :] < c[:, None]
            equal = np.array_equal(c, c2) and np.array_equal(o[live], o2[live]) and np.array_equal(s[live].view(np.uint32), s2[live].view(np.uint32))
            row = [name, str(handle.count), str(span), str(nq), f"{ms['rowlist']:.3f}", f"{ms['tile']:.3f}", f"{ms['wide']:.3f}", f"{ms['parent']:.3f}",
                   f"{ms['parent2']:.3f}", f"{max(both) - min(both):.3f}", f"{ms['default']:.3f}", str(routes["default"]), f"{ms['tile'] / ms['wide']:.2f}",
                   f"{ms['default'] - min(ms['parent'], ms['parent2']):+.3f}", f"{ms['unmasked']:.3f}" if "unmasked" in ms else "",
                   f"{ms['wide'] / ms['unmasked']:.2f}" if "unmasked" in ms else "", "yes" if equal else "NO"]
            lines.append("| " + " | ".join(row) + " |")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
