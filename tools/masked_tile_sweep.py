"""Masked batches: the gather route (the mask's row list, eight queries per pass: tavb_search_subset_batch_resident) against the 32/64-query tile
with the bit test in its admission path (tavb_search_masked_batch), and what the default options pick (tavb_plan_masked), in one process on
one corpus (default 1M x 1536, fp16 and fp32) at masks of 1, 10, 50 and 100 % allowed rows, random and contiguous, under batches of 8, 32, 64,
256 and 1024 queries.

  gather    fuzzy_lookup_embeddings_masked(Q, RowMask) with mask_tile = 0 -- the code as it was before the tile route: this leg is the parent's time
  gather2   the same leg again, interleaved; `spread` = the range (slowest - fastest call) of the two legs' timed calls in this run
  tile      mask_tile = 2
  default   mask_tile = 1 with the shipped mask_tile_min_bytes / mask_tile_pct
  unmasked  (100 % rows only) fuzzy_lookup_embeddings of the same batch: the lookup the all-ones mask sits next to

Legs are interleaved (one call of each per round, `--reps` rounds after one warm-up round), medians of host-synchronous calls in ms, all
through `as_arrays=True`.  The tile's answers are compared with the gather route's: same counts, scores within 1e-5, and the share of (query,
rank) slots that hold the same ordinal.  Writes a markdown report (default profiles/r14_masked_tile.md).

  python tools/masked_tile_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--densities 0.01,0.1,0.5,1] [--batches 8,32,64,256,1024] [--k 10] [--reps 5] [--out ...]
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


def agreement(a, b) -> tuple[bool, float]:
    """(counts equal and scores within 1e-5 slot by slot, share of live slots with the same ordinal)"""
    (oa, sa, ca), (ob, sb, cb) = a, b
    if not np.array_equal(ca, cb):
        return False, 0.0
    live = np.arange(oa.shape[1])[None, :] < ca[:, None]
    close = bool((np.abs(sa[live].astype(np.float64) - sb[live].astype(np.float64)) <= 1e-5).all())
    return close, float((oa[live] == ob[live]).mean()) if live.any() else 1.0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--densities", default="0.01,0.1,0.5,1")
    ap.add_argument("--batches", default="8,32,64,256,1024")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_masked_tile.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    batches = [int(x) for x in args.batches.split(",")]
    k = args.k
    lines = [
        "# Masked batches: the gather route against the 32/64-query tile",
        "",
        "`" + " ".join(["python", "tools/masked_tile_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)}, max_hits = {k}, min_score = 0; legs interleaved, medians of {args.reps} host-synchronous",
        "calls after a warm-up round, ms.  `gather` is the route as it was before the tile route existed (mask_tile = 0): the parent's time of the",
        "cell.  `gather2` = the same leg a second time; `spread` = slowest - fastest of the two legs' timed calls.  `default` = mask_tile = 1 with the shipped thresholds; `route` = what it",
        "took (1 = gather, 2 = tile).  `unmasked` (100 % only) = fuzzy_lookup_embeddings of the same batch.  `agree` = the tile's counts equal the",
        "gather route's and its scores are within 1e-5; `same ordinals` = share of result slots holding the same row.",
        "",
    ]
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        qs = host_queries(max(batches), args.dim, 131)
        lines += [f"## {dtype}", "",
                  "| mask | rows allowed | span | queries | gather | gather2 | spread | tile | default | route | gather / tile | default / gather | unmasked | tile / unmasked | agree | same ordinals |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for dens in (float(x) for x in args.densities.split(",")):
            kinds = ("all",) if dens >= 1 else ("random", "contiguous")
            for kind in kinds:
                if kind == "random":
                    mask = np.random.default_rng(int(dens * 1000)).random(args.rows) < dens
                elif kind == "contiguous":  # unaligned ends
                    lo = int(0.3 * args.rows) + 7
                    mask = np.zeros(args.rows, dtype=bool)
                    mask[lo: lo + int(dens * args.rows)] = True
                else:
                    mask = np.ones(args.rows, dtype=bool)
                handle = vb.row_mask(mask)
                span = handle.span[1] + 1 - handle.span[0] // 256 * 256
                for nq in batches:
                    q = qs[:nq]

                    def leg(mode):
                        def run():
                            eng.set_option("mask_tile", mode)
                            return vb.fuzzy_lookup_embeddings_masked(q, handle, k, 0.0, as_arrays=True)
                        return run

                    routes = {}

                    def default_leg():
                        r = leg(1)()
                        routes["default"] = eng.get_option("masked_route")
                        return r

                    legs = {"gather": leg(0), "tile": leg(2), "gather2": leg(0), "default": default_leg}
                    if dens >= 1:
                        legs["unmasked"] = lambda: vb.fuzzy_lookup_embeddings(q, k, 0.0, as_arrays=True)
                    ms, out, calls = interleaved(legs, args.reps)
                    both = calls["gather"] + calls["gather2"]  # the spread of the repeated gather legs: the range of their calls
                    eng.set_option("mask_tile", 1)
                    ok, same = agreement(out["tile"], out["gather"])
                    g = ms["gather"]
                    row = [f"{kind} {dens:g}", str(handle.count), str(span), str(nq), f"{g:.3f}", f"{ms['gather2']:.3f}", f"{max(both) - min(both):.3f}", f"{ms['tile']:.3f}",
                           f"{ms['default']:.3f}", str(routes["default"]), f"{g / ms['tile']:.2f}", f"{ms['default'] / g:.2f}",
                           f"{ms['unmasked']:.3f}" if "unmasked" in ms else "", f"{ms['tile'] / ms['unmasked']:.2f}" if "unmasked" in ms else "",
                           "yes" if ok else "NO", f"{same:.4f}"]
                    lines.append("| " + " | ".join(row) + " |")
                    print(lines[-1], flush=True)
        lines.append("")
        vb.clear()
        del vb, corpus
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
