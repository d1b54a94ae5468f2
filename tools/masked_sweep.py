"""Masked-lookup sweep: the mask expansion (tavb_mask_expand) and the batched resident subset (tavb_search_subset_batch_resident) against
the subset calls they stand next to, in one process, on one corpus (default 1M x 1536 fp16) at mask densities 1 %, 10 % and 50 %.

  expand   tavb_mask_expand alone over bits already on the device (count known), host-synchronous
  devmask  row_mask(torch.bool tensor on the device): pack, count, write -- two library calls more than `expand`, the mask never on the host
  masked   fuzzy_lookup_embedding_masked(q, RowMask)            one query, only the query travels
  subset   fuzzy_lookup_embedding_in_subset(q, the same list)   one query over the cached resident row list of the same rows
  batch    fuzzy_lookup_embeddings_masked(Q queries, RowMask)   one call, Q = 8 and 32
  loop     Q sequential fuzzy_lookup_embedding_in_subset calls over the cached list
  fresh    a fresh numpy mask through fuzzy_lookup_embedding_masked against a fresh ordinal list of the same rows through
           fuzzy_lookup_embedding_in_subset: conversion and upload on both sides

`fuzzy_lookup_embedding_in_subset` is the code of the commit before the masked lookups (they add to the class and change none of its
routes), so "subset" and "loop" are that commit's numbers measured in the same process on the same box.  Medians of host-synchronous
calls in ms; masked and subset answers are compared bit for bit.  Writes a markdown report (default profiles/r09_masked.md).

  python tools/masked_sweep.py [--rows 1000000] [--dtype fp16] [--densities 0.01,0.1,0.5] [--k 10] [--reps 9] [--out profiles/r09_masked.md]
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


def timed(fn, reps):
    fn()  # warm-up (workspaces, the subset cache)
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtype", default="fp16")
    ap.add_argument("--densities", default="0.01,0.1,0.5")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_masked.md"))
    args = ap.parse_args()
    import torch

    shown = [a for i, a in enumerate(sys.argv[1:]) if a != "--out" and (i == 0 or sys.argv[i] != "--out")]  # (where the report goes is not part of the measurement)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=args.dtype)
    eng0 = _native.Engine(0)
    corpus = make_device_corpus(eng0, args.rows, args.dim, 4242, args.dtype)
    eng0.close()
    vb.adopt_device_corpus(corpus)
    eng = vb.engine
    qs = host_queries(32, args.dim, 131)
    k = args.k
    lines = [
        "# Masked lookups: expansion, single query, batch, fresh mask",
        "",
        "`" + " ".join(["python", "tools/masked_sweep.py"] + shown) + "`",
        "",
        f"{args.rows} x {args.dim} {args.dtype} rows on {torch.cuda.get_device_name(0)}, max_hits = {k}, min_score = 0, medians of {args.reps} host-synchronous calls, ms.",
        "`subset` / `loop` = `fuzzy_lookup_embedding_in_subset` over its cached resident list of the same rows (the routes as they were before the",
        "masked lookups were added: this change leaves them as they are).",
        "",
        "| density | rows allowed | expand | devmask | masked 1q | subset 1q | masked / subset | expand / masked | batch 8 | loop 8 | loop / batch | batch 32 | loop 32 | loop / batch | fresh mask | fresh list | list / mask | bit-identical |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for dens in (float(x) for x in args.densities.split(",")):
        mask = np.random.default_rng(int(dens * 1000)).random(args.rows) < dens
        flat = np.flatnonzero(mask)
        ordinals = flat.tolist()  # what a consumer hands fuzzy_lookup_embedding_in_subset
        bits = torch.from_numpy(_native.pack_mask_bits(mask).view(np.int32)).to("cuda:0")
        t_expand, _ = timed(lambda: eng.expand_mask_bits(bits, args.rows, cap=len(flat)), args.reps)
        dev_mask = torch.from_numpy(mask).to("cuda:0")
        t_devmask, dev_handle = timed(lambda: vb.row_mask(dev_mask), args.reps)
        handle = vb.row_mask(mask)
        assert torch.equal(dev_handle.dev_rows, handle.dev_rows)
        t_masked, a1 = timed(lambda: vb.fuzzy_lookup_embedding_masked(qs[0], handle, k, 0.0), args.reps)
        t_subset, b1 = timed(lambda: vb.fuzzy_lookup_embedding_in_subset(qs[0], ordinals, k, 0.0), args.reps)
        ok = same([a1], [b1])
        row = [f"{dens:g}", str(len(flat)), f"{t_expand:.3f}", f"{t_devmask:.3f}", f"{t_masked:.3f}", f"{t_subset:.3f}", f"{t_masked / t_subset:.2f}", f"{t_expand / t_masked:.2f}"]
        for nq in (8, 32):
            t_batch, ab = timed(lambda: vb.fuzzy_lookup_embeddings_masked(qs[:nq], handle, k, 0.0), args.reps)
            t_loop, bb = timed(lambda: [vb.fuzzy_lookup_embedding_in_subset(q, ordinals, k, 0.0) for q in qs[:nq]], max(3, args.reps // 3))
            ok = ok and same(ab, bb)
            row += [f"{t_batch:.3f}", f"{t_loop:.3f}", f"{t_loop / t_batch:.2f}"]
        t_fresh_mask, af = timed(lambda: vb.fuzzy_lookup_embedding_masked(qs[1], mask.copy(), k, 0.0), max(3, args.reps // 3))
        t_fresh_list, bf = timed(lambda: vb.fuzzy_lookup_embedding_in_subset(qs[1], list(ordinals), k, 0.0), max(3, args.reps // 3))
        ok = ok and same([af], [bf])
        row += [f"{t_fresh_mask:.3f}", f"{t_fresh_list:.3f}", f"{t_fresh_list / t_fresh_mask:.1f}", "yes" if ok else "NO"]
        lines.append("| " + " | ".join(row) + " |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
