#!/usr/bin/env python3
"""`fuzzy_lookup_rows` natively (tavb_search_rows) against its host route (engine option "rows_query" = 0) in ONE process, legs interleaved,
three rounds, every cell compared for equality; then `near_duplicate_pairs` over a duplicate-heavy corpus.  Writes profiles/r29_lookup_rows.md.

    python tools/lookup_rows_sweep.py [--rows 1000000] [--dim 1536] [--pairs-rows 100000] [--out profiles/r29_lookup_rows.md]

Cells: corpus dtype fp16 / fp32, n = 1 / 8 / 64 / 1024 / 16384 rows, max_hits 10 / 100.  A cell where the native call is slower than the
host route beyond the spread of the host leg's rounds is named; no routing rule is fitted."""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.fakes import NullModel  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase  # noqa: E402

NS = (1, 8, 64, 1024, 16384)
KS = (10, 100)
ROUNDS = 3


def corpus(rows: int, dim: int, seed: int, dup_every: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = np.empty((rows, dim), dtype=np.float32)
    for lo in range(0, rows, 65536):
        hi = min(rows, lo + 65536)
        v[lo:hi] = rng.standard_normal((hi - lo, dim), dtype=np.float32)
        v[lo:hi] /= np.linalg.norm(v[lo:hi], axis=1, keepdims=True)
    if dup_every:  # duplicate-heavy: every dup_every-th row is a near copy of an earlier one
        src = rng.integers(0, rows, size=rows // dup_every)
        dst = np.arange(dup_every - 1, rows, dup_every)[: len(src)]
        w = v[src] + 0.01 * rng.standard_normal((len(src), dim), dtype=np.float32) / np.sqrt(dim)
        v[dst] = w / np.linalg.norm(w, axis=1, keepdims=True)
    return v


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def same(a, b) -> bool:
    return len(a) == len(b) and all([(h.item, h.score) for h in x] == [(h.item, h.score) for h in y] for x, y in zip(a, b))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--pairs-rows", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_lookup_rows.md"))
    args = ap.parse_args()
    lines = ["# r29: fuzzy_lookup_rows, native (tavb_search_rows) against the host route (rows_query = 0)", "",
             f"corpus {args.rows} x {args.dim}; ms per call, the lowest of {ROUNDS} interleaved rounds (host leg's spread in brackets); `equal`: the lists are identical", "",
             "| dtype | n | max_hits | native ms | host ms [min .. max] | host / native | equal |", "|---|---|---|---|---|---|---|"]
    slower = []
    v = corpus(args.rows, args.dim, 29)
    for dtype in ("fp16", "fp32"):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
        vb.add_embeddings(None, v)
        eng = vb.engine
        rng = np.random.default_rng(1)
        for n in NS:
            asked = rng.integers(0, args.rows, size=n)
            for k in KS:
                legs = {0: [], 1: []}
                answers = {}
                for rnd in range(ROUNDS + 1):  # (round 0 warms both legs up)
                    for native in (1, 0):
                        eng.set_option("rows_query", native)
                        ms, out = timed(lambda: vb.fuzzy_lookup_rows(asked, k, 0.0))
                        if rnd:
                            legs[native].append(ms)
                        answers[native] = out
                eng.set_option("rows_query", 1)
                nat, host = min(legs[1]), min(legs[0])
                eq = same(answers[1], answers[0])
                lines.append(f"| {dtype} | {n} | {k} | {nat:.3f} | {host:.3f} [{min(legs[0]):.3f} .. {max(legs[0]):.3f}] | {host / nat:.2f} | {'yes' if eq else 'NO'} |")
                if nat > max(legs[0]):
                    slower.append(f"{dtype} n={n} max_hits={k}: native {nat:.3f} ms, host {min(legs[0]):.3f} .. {max(legs[0]):.3f} ms")
                print(lines[-1], flush=True)
        eng.close()
        del vb
    del v
    lines += ["", "Cells where the native call is slower than every round of the host leg:", ""] + ([f"- {s}" for s in slower] or ["- none"])
    # ---- near_duplicate_pairs over a duplicate-heavy corpus
    w = corpus(args.pairs_rows, args.dim, 30, dup_every=3)
    lines += ["", f"## near_duplicate_pairs(0.95, 16) over {args.pairs_rows} x {args.dim}, every third row a near copy", "",
              "| dtype | native ms | host ms | pairs | equal |", "|---|---|---|---|---|"]
    for dtype in ("fp16", "fp32"):
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
        vb.add_embeddings(None, w)
        eng = vb.engine
        res = {}
        for native in (1, 0):
            eng.set_option("rows_query", native)
            res[native] = timed(lambda: vb.near_duplicate_pairs(0.95, 16))
        eq = all(np.array_equal(a, b) for a, b in zip(res[1][1], res[0][1]))
        lines.append(f"| {dtype} | {res[1][0]:.1f} | {res[0][0]:.1f} | {len(res[1][1][0])} | {'yes' if eq else 'NO'} |")
        print(lines[-1], flush=True)
        eng.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
