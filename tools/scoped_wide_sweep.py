"""Scoped-wide sweep: `fuzzy_lookup_embeddings_scoped` on the 128/256-query filter tile + rescoring (engine option scope_wide = 2:
tavb_search_scoped_wide) against the routes a library without it takes, in one process, on one fp16 corpus (default 1M x 1536), for batches of
128 / 256 / 1024 queries, max_hits 10 and 100, scopes of 10 % / 50 % / 100 % of the rows and the three families of tools/scoped_tile_sweep.py
(same-rows, independent, disjoint).  Legs, interleaved within every round:

  wide       scope_wide = 2
  row list   scope_wide = 0, scope_tile = 0 (tavb_search_scoped_batch)
  tile       scope_wide = 0, scope_tile = 2 (tavb_search_scoped_tile; max_hits <= 64 only)
  one mask   same-rows cells only: `fuzzy_lookup_embeddings_masked` over ONE of the handles on the one-mask wide route (mask_wide = 2) -- what
             the plane test itself costs -- and, for the 100 % cell, the unmasked `fuzzy_lookup_embeddings`

`before` is the leg a library without the wide route takes at its defaults: the tile where tavb_plan_scoped says so (max_hits <= 64), else the
row list.  A cell reports the median over --rounds rounds of each leg (each the median of --reps host-synchronous calls), before / wide (above
1 the wide route wins), the spread of the `before` leg's rounds ((max - min) / median), what tavb_plan_scoped_wide says at the default
thresholds, and whether a cell the plan sends to the wide route is slower than `before` beyond that spread.  The wide and the row-list answers
are compared bit for bit.  Also: the plane build of 256 scopes next to the 256-query wide call that holds it, and the planes' workspace.

  python tools/scoped_wide_sweep.py [--rows 1000000] [--batches 128,256,1024] [--ks 10,100] [--reps 2] [--rounds 3] [--out profiles/r22_scoped_wide.md]
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
from tools.scoped_batch_sweep import kept_tail, median_ms  # noqa: E402
from tools.scoped_tile_sweep import FAMILIES, scopes_for  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native  # noqa: E402


def identical(a, b) -> int:
    """queries whose answers agree bit for bit: ordinals and float32 scores"""
    return sum([(r.item, np.float32(r.score).tobytes()) for r in x] == [(r.item, np.float32(r.score).tobytes()) for r in y] for x, y in zip(a, b))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--batches", default="128,256,1024")
    ap.add_argument("--shares", default="0.1,0.5,1.0")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_scoped_wide.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]
    batches = [int(x) for x in args.batches.split(",")]
    ks = [int(x) for x in args.ks.split(",")]
    lines = [
        "# Scoped batches on the 128/256-query filter tile against the row list and the 32/64-query tile",
        "",
        "`" + " ".join(["python", "tools/scoped_wide_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} fp16 rows on {torch.cuda.get_device_name(0)}, min_score = 0, host-synchronous calls of",
        "`fuzzy_lookup_embeddings_scoped(queries, handles)`, ms.  `wide` = scope_wide = 2 (tavb_search_scoped_wide); `row list` = scope_wide = 0, scope_tile = 0;",
        "`tile` = scope_wide = 0, scope_tile = 2 (max_hits <= 64); `one mask` = the one-mask wide route over one of the equal scopes (same-rows cells);",
        "`unmasked` = the plain batched lookup (the 100 % same-rows cells).  `before` = the leg a library without the wide route takes at its defaults (the",
        f"tile where tavb_plan_scoped says so, else the row list).  The legs are interleaved: {args.rounds} rounds of the median of {args.reps} calls per leg; the table",
        "has the median over the rounds, before / wide (above 1: the wide route is faster), the spread = (max - min) / median of the `before` leg's rounds,",
        "`plan` = what tavb_plan_scoped_wide says at the default thresholds (128 MiB per pass, 100 %), and `same` = queries whose wide answers equal the",
        "row list's bit for bit.",
        "",
        "| family | share | queries | max_hits | wide | row list | tile | one mask | unmasked | before | spread | before / wide | plan | planned and slower beyond the spread | same |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype="fp16")
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, "fp16")
    eng0.close()
    vb.adopt_device_corpus(corpus)
    eng = vb.engine
    qs = host_queries(max(batches), args.dim, 131)
    legs_opts = {"wide": (("scope_wide", 2), ("scope_tile", 0)), "list": (("scope_wide", 0), ("scope_tile", 0)), "tile": (("scope_wide", 0), ("scope_tile", 2))}
    routes = {"wide": 6, "list": 4, "tile": 5}

    def use(leg):
        for name, val in legs_opts[leg]:
            eng.set_option(name, val)

    cells, build = [], None
    for family in FAMILIES:
        for share in (float(x) for x in args.shares.split(",")):
            every = scopes_for(vb, family, share, max(batches), args.rows, int(share * 1000) + 7)
            if every is None:
                continue
            for nq in batches:
                handles = every[:nq]
                order = vb._scoped_order(handles)
                first, last = min(handles[i].span[0] for i in order), max(handles[i].span[1] for i in order)
                span = last + 1 - first // 256 * 256
                counts = [handles[i].count for i in order]
                for k in ks:
                    call = lambda: vb.fuzzy_lookup_embeddings_scoped(qs[:nq], handles, k, 0.0)  # noqa: E731
                    legs = {"wide": call, "list": call}
                    if k <= 64:
                        legs["tile"] = call
                    if family == "same-rows":
                        legs["mask"] = lambda: vb.fuzzy_lookup_embeddings_masked(qs[:nq], handles[0], k, 0.0)  # noqa: E731
                        if share >= 1.0:
                            legs["plain"] = lambda: vb.fuzzy_lookup_embeddings(qs[:nq], k, 0.0)  # noqa: E731
                    eng.set_option("mask_wide", 2)
                    answers = {}
                    for leg, fn in legs.items():  # warm-up: workspaces; the routes
                        if leg in legs_opts:
                            use(leg)
                        answers[leg] = fn()
                        if leg in routes:
                            assert eng.get_option("masked_route") == routes[leg], (leg, eng.get_option("masked_route"))
                    times = {leg: [] for leg in legs}
                    for _ in range(args.rounds):
                        for leg, fn in legs.items():
                            if leg in legs_opts:
                                use(leg)
                            times[leg].append(median_ms(fn, args.reps)[0])
                    med = {leg: float(np.median(t)) for leg, t in times.items()}
                    plan_tile = k <= 64 and _native.plan_scoped(nq, k, args.dim, eng.dtype, _native.scoped_gather_rows(counts), span)
                    plan = _native.plan_scoped_wide(nq, k, args.dim, eng.dtype, _native.scoped_gather_rows(counts, 4 if k > 64 else 8), span)
                    before = "tile" if plan_tile else "list"
                    spread = (max(times[before]) - min(times[before])) / med[before]
                    slower = plan and med["wide"] > med[before] * (1.0 + spread)
                    same = identical(answers["wide"], answers["list"])
                    cell = lambda leg: f"{med[leg]:.3f}" if leg in med else "-"  # noqa: E731
                    lines.append(f"| {family} | {share:g} | {nq} | {k} | {cell('wide')} | {cell('list')} | {cell('tile')} | {cell('mask')} | {cell('plain')} | "
                                 f"{'tile' if plan_tile else 'row list'} {med[before]:.3f} | {100 * spread:.1f} % | {med[before] / med['wide']:.2f} | "
                                 f"{'wide' if plan else 'no'} | {'YES' if slower else 'no'} | {same}/{nq} |")
                    cells.append({"family": family, "share": share, "nq": nq, "k": k, **med, "before": med[before], "plan": plan, "slower": slower, "same": same})
                    print(lines[-1], flush=True)
            if family == "independent" and share == 0.5 and len(every) >= 256:  # the plane build next to the wide call that holds it
                bits = [h.dev_bits for h in every[:256]]
                sp = (min(h.span[0] for h in every[:256]), max(h.span[1] for h in every[:256]))
                dq = torch.from_numpy(np.ascontiguousarray(qs[:256])).cuda()

                def planes():
                    eng.scope_planes(bits, span=sp)
                    eng.synchronize()

                def wide():
                    eng.search_scoped_wide_device(dq, bits, 10, 0.0, span=sp)
                    eng.synchronize()

                planes(), wide()
                blocks, words, _ = _native.scope_plane_shape(256, *sp)
                build = (median_ms(planes, 9)[0], median_ms(wide, 9)[0], blocks * words * 4)
            del every
    for name, val in (("scope_wide", 1), ("scope_tile", 1), ("mask_wide", 1)):
        eng.set_option(name, val)
    planned = [c for c in cells if c["plan"]]
    lines += ["", "## Reading", "",
              f"- {len(cells)} cells; the plan sends {len(planned)} to the wide route at the default thresholds; {sum(c['slower'] for c in cells)} of those are slower "
              "than `before` beyond that leg's spread.",
              f"- wide faster than `before` (ratio >= 1.00) in {sum(c['before'] / c['wide'] >= 0.995 for c in cells)} of {len(cells)} cells; of the cells the plan keeps "
              f"off the wide route, it would have been faster in {sum((not c['plan']) and c['before'] / c['wide'] >= 0.995 for c in cells)}.",
              f"- answers equal to the row list's bit for bit in {sum(c['same'] == c['nq'] for c in cells)} of {len(cells)} cells."]
    for c in cells:
        if c["slower"]:
            lines.append(f"- PLANNED AND SLOWER: {c['family']} scopes of {100 * c['share']:g} %, {c['nq']} queries, max_hits {c['k']} -- {c['wide']:.3f} ms against {c['before']:.3f} ms.")
    for family in FAMILIES:
        r = [c["before"] / c["wide"] for c in cells if c["family"] == family and c["plan"]]
        if r:
            lines.append(f"- {family}, planned cells: before / wide {min(r):.2f} -- {max(r):.2f} over {len(r)} cells.")
    r = [c["wide"] / c["mask"] for c in cells if "mask" in c]
    if r:
        lines.append(f"- the plane test: wide / one mask {min(r):.2f} -- {max(r):.2f} over the {len(r)} same-rows cells (planes built per call, 32 plane words per admitting block).")
    if build:
        lines += ["", "## Plane build next to one wide call", "",
                  "256 independent 50 % scopes: `tavb_scope_planes` alone (launch to synchronise) and `tavb_search_scoped_wide_device` of the 256 queries (max_hits 10), which",
                  "builds the same planes, filters, selects and rescores; host timers around synchronised calls, median of 9, ms.", "",
                  "| plane build | wide call | build / call | planes of the 256 queries |", "|---|---|---|---|",
                  f"| {build[0]:.3f} | {build[1]:.3f} | {100 * build[0] / build[1]:.0f} % | {build[2] / 2**20:.1f} MiB |"]
    tail = kept_tail(args.out)
    text = "\n".join(lines + ([""] + tail if tail else [])).rstrip("\n") + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
