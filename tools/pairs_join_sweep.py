#!/usr/bin/env python3
"""`similarity_join` / `near_duplicate_pairs` on the self-join (tavb_join_pairs) against the row lookups (engine option "pairs_join" = 0) in
ONE process, legs interleaved, three rounds, every answer compared bit for bit.  Writes profiles/r30_pairs_join.md.

    python tools/pairs_join_sweep.py [--sizes 4000,8000,10000,100000,1000000] [--dim 1536] [--budget-s 600] [--out profiles/r30_pairs_join.md]

Corpus: the `pairs_corpus` recipe of tests/lookup_rows_cases.py scaled up -- unit gaussian rows, about 1 % of them planted as exact or near
copies of another row.  Cells: fp16 and fp32, min_score 0.95, max_per_row 16.  Per cell: ms (the lowest of the rounds, the row lookups'
spread in brackets), the ratio, candidates against pairs, achieved TFLOP/s on N (N + 1) / 2 x 2 x dim flops and the fraction of the dense fp16
peak at the board clock bench.py's sampler reads.  The row lookups' leg of a cell is cut by --budget-s: a leg that would not finish is
reported as such, never extrapolated.  The default of "pairs_join_min_rows" is the smallest swept row count at which the join beats every
round of the row lookups; no further rule is fitted."""

from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import MFMA_F16_PEAK_TFLOPS, HwmonSampler  # noqa: E402
from tests.fakes import NullModel  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase  # noqa: E402

ROUNDS = 3
MIN_SCORE = 0.95


def corpus(rows: int, dim: int, seed: int = 30) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = np.empty((rows, dim), dtype=np.float32)
    for lo in range(0, rows, 65536):
        hi = min(rows, lo + 65536)
        v[lo:hi] = rng.standard_normal((hi - lo, dim), dtype=np.float32)
        v[lo:hi] /= np.linalg.norm(v[lo:hi], axis=1, keepdims=True)
    n_pairs = max(rows // 200, 1)  # two rows per pair: about 1 % of the rows
    picks = rng.permutation(rows)[: 2 * n_pairs].reshape(n_pairs, 2)
    near = np.arange(n_pairs) % 3 != 0
    w = v[picks[:, 0]] + near[:, None] * (0.02 * rng.standard_normal((n_pairs, dim), dtype=np.float32) / np.sqrt(dim))
    v[picks[:, 1]] = w / np.linalg.norm(w, axis=1, keepdims=True)
    return v


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def same(a, b) -> bool:
    return all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


def main() -> None:
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4000,8000,10000,100000,1000000")
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--budget-s", type=float, default=600.0, help="a cell's row-lookup leg is not started when one round is predicted beyond this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r30_pairs_join.md"))
    args = ap.parse_args()
    sizes = [int(x) for x in args.sizes.split(",")]
    lines = ["# r30: near_duplicate_pairs / similarity_join, the self-join (tavb_join_pairs) against the row lookups (pairs_join = 0)", "",
             f"rows x {args.dim}, about 1 % of the rows planted, min_score {MIN_SCORE}, max_per_row 16; ms per call, the lowest of {ROUNDS} interleaved rounds "
             "(row lookups: their spread in brackets); `equal`: (i, j, score bits) identical", "",
             "| dtype | rows | join ms | lookups ms [min .. max] | lookups / join | candidates | pairs | TFLOP/s | of fp16 peak at sclk | sclk MHz | equal |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    wins: dict[str, list[int]] = {"fp16": [], "fp32": []}
    rate = {"fp16": None, "fp32": None}  # ms per row^2 of the row lookups, from the cells that ran: predicts the next cell's leg
    for rows in sizes:
        v = corpus(rows, args.dim)
        for dtype in ("fp16", "fp32"):
            vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), device=0, corpus_dtype=dtype)
            vb.add_embeddings(None, v)
            eng = vb.engine
            eng.set_option("pairs_join_min_rows", 1)
            predicted = None if rate[dtype] is None else rate[dtype] * rows * rows / 1e3
            run_old = predicted is None or predicted * (ROUNDS + 1) <= args.budget_s
            legs = {0: [], 1: []}
            answers = {}
            hw = HwmonSampler(torch, 0)
            for rnd in range(ROUNDS + 1):  # (round 0 warms both legs up)
                for join in (1, 0):
                    if not join and not run_old:
                        continue
                    eng.set_option("pairs_join", join)
                    if join and rnd == ROUNDS:
                        with hw:
                            ms, out = timed(lambda: vb.near_duplicate_pairs(MIN_SCORE, 16))
                    else:
                        ms, out = timed(lambda: vb.near_duplicate_pairs(MIN_SCORE, 16))
                    if join:
                        assert eng.get_option("pairs_join_launches") >= 1
                        cand = eng.get_option("pairs_join_candidates")
                    if rnd:
                        legs[join].append(ms)
                    answers[join] = out
            eng.set_option("pairs_join", 1)
            jn = min(legs[1])
            tflops = rows * (rows + 1) / 2 * 2 * args.dim / (jn * 1e-3) / 1e12
            clk = hw.summary()
            sclk = clk["sclk_mhz"] if clk else 0.0
            frac = tflops / (MFMA_F16_PEAK_TFLOPS * sclk / 2400.0) if sclk else float("nan")
            if run_old:
                old = min(legs[0])
                rate[dtype] = old / rows / rows
                eq = "yes" if same(answers[1], answers[0]) else "NO"
                old_text, ratio = f"{old:.1f} [{min(legs[0]):.1f} .. {max(legs[0]):.1f}]", f"{old / jn:.2f}"
                if jn < min(legs[0]):
                    wins[dtype].append(rows)
            else:
                old_text, ratio, eq = f"not run: predicted {predicted:.0f} s a round, beyond the budget", "-", "-"
            lines.append(f"| {dtype} | {rows} | {jn:.3f} | {old_text} | {ratio} | {cand} | {len(answers[1][0])} | {tflops:.1f} | {frac:.3f} | {sclk:.0f} | {eq} |")
            print(lines[-1], flush=True)
            eng.close()
            del vb
        del v
    lines += ["", "Smallest swept row count at which the join beats every round of the row lookups (the default of `pairs_join_min_rows` is the larger of the two, "
              "and stays above 2000):", ""] + [f"- {d}: {min(w) if w else 'none'}" for d, w in wins.items()]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
