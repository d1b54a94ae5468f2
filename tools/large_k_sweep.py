"""Large-k sweep: exact device top-k (tavb_search_topk) against the emit-all route it replaces (large_k = 0: tavb_search_all, host sort,
one pass per query) and against the K = 256 fused lookup, in one process.

For K in {256, 257, 1000, 4096, MAX_LARGE_K} x corpora (10k fp32, 1M fp32, 10M fp16; 1536 wide) x nq in {1, 8, 32} at min_score 0:
  new   VectorBase.fuzzy_lookup_embeddings / fuzzy_lookup_embedding with large_k = 1 (the default)
  old   the same call with large_k = 0 (the per-query emit-all loop)
  k256  the same queries at max_hits = 256 (the fused select-while-streaming kernels)
Medians of host-synchronous calls in ms; the answers of new and old are compared bit for bit (ordinals and score bits).  Prints one markdown
table (the source of profiles/r07_large_k.md).

  python tools/large_k_sweep.py [--sizes 10k,1m,10m] [--ks 256,257,1000,4096,16384] [--nqs 1,8,32] [--reps 5] [--old-max-nq 8]
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

SIZES = {"10k": (10_000, "fp32"), "1m": (1_000_000, "fp32"), "10m": (10_000_000, "fp16")}


def timed(fn, reps):
    fn()  # warm-up (workspaces, LDS attributes)
    ts = []
    out = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, out


def flat(res):
    """lists of ScoredInt (one list per query) -> (ordinals, score bits)"""
    items = np.array([r.item for q in res for r in q], dtype=np.int64)
    bits = np.array([r.score for q in res for r in q], dtype=np.float32).view(np.uint32)
    return items, bits, [len(q) for q in res]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10k,1m,10m")
    ap.add_argument("--ks", default=f"256,257,1000,4096,{_native.MAX_LARGE_K}")
    ap.add_argument("--nqs", default="1,8,32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--old-max-nq", type=int, default=32, help="skip the old route above this many queries on corpora of 10M+ rows (it is one pass and one host sort per query)")
    args = ap.parse_args()
    ks = [int(x) for x in args.ks.split(",")]
    nqs = [int(x) for x in args.nqs.split(",")]
    print("| corpus | nq | K | new ms | old ms | K=256 ms | new / K=256 | old / new | refine rounds | bit-identical |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for size in args.sizes.split(","):
        rows, dtype = SIZES[size]
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
        eng0 = _native.Engine(0)
        corpus = make_device_corpus(eng0, rows, 1536, 4242 + rows % 1000, dtype)
        eng0.close()
        vb.adopt_device_corpus(corpus)
        eng = vb.engine
        for nq in nqs:
            qs = host_queries(nq, 1536, 99 + nq)

            def call(k, large):
                eng.set_option("large_k", large)
                if nq == 1:
                    return [vb.fuzzy_lookup_embedding(qs[0], max_hits=k, min_score=0.0)]
                return vb.fuzzy_lookup_embeddings(qs, max_hits=k, min_score=0.0)

            t256, _ = timed(lambda: call(256, 1), args.reps)
            for k in ks:
                t_new, new = timed(lambda: call(k, 1), args.reps)
                rounds = eng.get_option("last_topk_refine")
                if k <= 256 or (rows >= 10_000_000 and nq > args.old_max_nq):
                    t_old, same = float("nan"), "-"
                else:
                    t_old, old = timed(lambda: call(k, 0), max(1, min(args.reps, 3)))
                    a, b = flat(new), flat(old)
                    same = "yes" if (a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])) else "NO"
                eng.set_option("large_k", 1)
                print(f"| {size} {dtype} | {nq} | {k} | {t_new:.3f} | {t_old:.3f} | {t256:.3f} | {t_new / t256:.2f} | {t_old / t_new:.1f} | {rounds} | {same} |",
                      flush=True)
        del vb, eng, corpus


if __name__ == "__main__":
    main()
