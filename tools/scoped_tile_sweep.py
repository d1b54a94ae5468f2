"""Scoped-tile sweep: `fuzzy_lookup_embeddings_scoped` on the 32/64-query MFMA tile (engine option scope_tile = 2: tavb_search_scoped_tile)
against the row-list scoped route (scope_tile = 0: tavb_search_scoped_batch, the path before the tile route existed) in one process, on one
corpus (default 1M x 1536, fp16 and fp32), for batches of 32 / 64 / 256 queries, scopes of 10 % / 50 % / 100 % of the rows and three families:

  same-rows    every query's scope has the same rows, each in a handle of its own (the SAME handle is no case here: the class hands it to
               `fuzzy_lookup_embeddings_masked`)
  independent  every scope drawn on its own
  disjoint     the rows dealt to floor(1 / share) slots, query q takes slot q mod slots (skipped where eight shares exceed the corpus)

The legs are interleaved: every round times the tile (median of --reps host-synchronous calls) and then the row list; a cell reports the
median over --rounds rounds of each, their ratio (row list / tile: above 1 the tile wins), the spread of the row-list leg's rounds
((max - min) / median), what tavb_plan_scoped says at the default thresholds, and whether a cell the plan sends to the tile is slower than
its row-list leg beyond that spread.  The answers are compared: queries with the same ordinals, and the largest score difference (the
tile's contract is not bit for bit).  Also times, per dtype, the plane build of 64 scopes next to the 64-query tile call that holds it.

  python tools/scoped_tile_sweep.py [--rows 1000000] [--dtypes fp16,fp32] [--k 10] [--reps 3] [--rounds 3] [--out profiles/r21_scoped_tile.md]
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
from tools.scoped_batch_sweep import KEEP, kept_tail, median_ms  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402

FAMILIES = ("same-rows", "independent", "disjoint")


def scopes_for(vb, family: str, share: float, nq: int, rows: int, seed: int):
    """nq RowMask handles, or None where the family has no such cell."""
    rng = np.random.default_rng(seed)
    if family == "same-rows":
        m = rng.random(rows) < share
        return [vb.row_mask(m.copy()) for _ in range(nq)]
    if family == "independent":
        return [vb.row_mask(rng.random(rows) < share) for _ in range(nq)]
    if 8 * share > 1.0:
        return None
    slots = int(1.0 / share)
    slot = rng.integers(0, slots, rows)
    made = [vb.row_mask(slot == s) for s in range(min(slots, nq))]
    return [made[q % len(made)] for q in range(nq)]


def compare(a, b) -> tuple[int, float]:
    """(queries whose ordinals agree, the largest score difference at agreeing ranks)"""
    same = sum([r.item for r in x] == [r.item for r in y] for x, y in zip(a, b))
    diff = max((abs(r.score - s.score) for x, y in zip(a, b) for r, s in zip(x, y)), default=0.0)
    return same, diff


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--batches", default="32,64,256")
    ap.add_argument("--shares", default="0.1,0.5,1.0")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_scoped_tile.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    k = args.k
    batches = [int(x) for x in args.batches.split(",")]
    lines = [
        "# Scoped batches on the 32/64-query tile against the row-list scoped route",
        "",
        "`" + " ".join(["python", "tools/scoped_tile_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} rows on {torch.cuda.get_device_name(0)}, max_hits = {k}, min_score = 0, host-synchronous calls of",
        "`fuzzy_lookup_embeddings_scoped(queries, handles)`, ms.  `tile` = engine option scope_tile = 2 (tavb_search_scoped_tile), `row list` = scope_tile = 0",
        f"(tavb_search_scoped_batch).  The legs are interleaved: {args.rounds} rounds of (median of {args.reps} tile calls, median of {args.reps} row-list calls); the table has the",
        "median over the rounds, `row list / tile` (above 1: the tile is faster), the spread = (max - min) / median of each leg's rounds, `plan` = what",
        "tavb_plan_scoped says at the default thresholds (128 MiB per pass, 100 %), and `same` = queries whose ordinals agree between the legs / the",
        "largest score difference.",
        "",
        "| dtype | family | share | queries | tile | spread | row list | spread | row list / tile | plan | planned and slower beyond the spread | same |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    cells, builds = [], []
    for dtype in args.dtypes.split(","):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        qs = host_queries(max(batches), args.dim, 131)
        for family in FAMILIES:
            for share in (float(x) for x in args.shares.split(",")):
                every = scopes_for(vb, family, share, max(batches), args.rows, int(share * 1000) + 7)
                if every is None:
                    continue
                for nq in batches:
                    handles = every[:nq]
                    call = lambda: vb.fuzzy_lookup_embeddings_scoped(qs[:nq], handles, k, 0.0)  # noqa: E731
                    eng.set_option("scope_tile", 2)
                    a = call()  # warm-up: workspaces
                    assert eng.get_option("masked_route") == 5
                    eng.set_option("scope_tile", 0)
                    b = call()
                    assert eng.get_option("masked_route") == 4
                    tt, tl = [], []
                    for _ in range(args.rounds):
                        eng.set_option("scope_tile", 2)
                        tt.append(median_ms(call, args.reps)[0])
                        eng.set_option("scope_tile", 0)
                        tl.append(median_ms(call, args.reps)[0])
                    t, l = float(np.median(tt)), float(np.median(tl))
                    st, sl = (max(tt) - min(tt)) / t, (max(tl) - min(tl)) / l
                    order = vb._scoped_order(handles)
                    first, last = min(handles[i].span[0] for i in order), max(handles[i].span[1] for i in order)
                    plan = _native.plan_scoped(nq, k, args.dim, eng.dtype, _native.scoped_gather_rows([handles[i].count for i in order]), last + 1 - first // 256 * 256)
                    slower = plan and t > l * (1.0 + sl)
                    same, diff = compare(a, b)
                    lines.append(f"| {dtype} | {family} | {share:g} | {nq} | {t:.3f} | {100 * st:.1f} % | {l:.3f} | {100 * sl:.1f} % | {l / t:.2f} | "
                                 f"{'tile' if plan else 'row list'} | {'YES' if slower else 'no'} | {same}/{nq}, {diff:.1e} |")
                    cells.append({"dtype": dtype, "family": family, "share": share, "nq": nq, "tile": t, "list": l, "spread": sl, "plan": plan, "slower": slower})
                    print(lines[-1], flush=True)
                if family == "independent" and share == 0.5 and len(every) >= 64:  # the plane build next to the tile call that holds it
                    bits = [h.dev_bits for h in every[:64]]
                    span = (min(h.span[0] for h in every[:64]), max(h.span[1] for h in every[:64]))
                    dq = torch.from_numpy(np.ascontiguousarray(qs[:64])).cuda()

                    def planes():
                        eng.scope_planes(bits, span=span)
                        eng.synchronize()

                    def tile():
                        eng.search_scoped_tile_device(dq, bits, k, 0.0, span=span)
                        eng.synchronize()

                    planes(), tile()
                    builds.append((dtype, median_ms(planes, 9)[0], median_ms(tile, 9)[0]))
                del every
        eng.set_option("scope_tile", 1)
        del vb, corpus, eng
        torch.cuda.empty_cache()
    planned = [c for c in cells if c["plan"]]
    lines += ["", "## Reading", "",
              f"- {len(cells)} cells; the plan sends {len(planned)} to the tile at the default thresholds; {sum(c['slower'] for c in cells)} of those are slower than "
              "their row-list leg beyond that leg's spread.",
              f"- tile faster (row list / tile >= 1.00) in {sum(c['list'] / c['tile'] >= 0.995 for c in cells)} of {len(cells)} cells; of the cells the plan keeps on "
              f"the row list, the tile would have been faster in {sum((not c['plan']) and c['list'] / c['tile'] >= 0.995 for c in cells)}."]
    for c in cells:
        if c["slower"]:
            lines.append(f"- PLANNED AND SLOWER: {c['dtype']}, {c['family']} scopes of {100 * c['share']:g} %, {c['nq']} queries -- {c['tile']:.3f} ms against {c['list']:.3f} ms.")
    for family in FAMILIES:
        for dtype in sorted({c["dtype"] for c in cells}):
            r = [c["list"] / c["tile"] for c in cells if c["family"] == family and c["dtype"] == dtype]
            if r:
                lines.append(f"- {family}, {dtype}: row list / tile {min(r):.2f} -- {max(r):.2f} over {len(r)} cells.")
    lines += ["", "## Plane build next to one tile call", "",
              "64 independent 50 % scopes: `tavb_scope_planes` alone (launch to synchronise) and `tavb_search_scoped_tile_device` of the 64 queries, which builds the",
              "same planes and runs the tile's phases; host timers around synchronised calls, median of 9, ms.", "",
              "| dtype | plane build | tile call (planes + phases) | build / call |", "|---|---|---|---|"]
    lines += [f"| {d} | {p:.3f} | {t:.3f} | {100 * p / t:.0f} % |" for d, p, t in builds]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
