#!/usr/bin/env python3
"""Interleaved A/B of the 256-query filter tile's MFMA shapes (option mfma_shape 16 / 32) on a cfg3-like corpus: 10M x 1536 random fp16 rows,
1024 random queries, k = 32, min_score 0, in ONE process (same box, same corpus, same thermal state).  Both shapes' answers are compared over
all 1024 x 32 keys first; then AB_ROUNDS rounds of AB_STEPS lookups per shape, the order alternating per round; per-lookup wall time around
search_device and a synchronise.  Prints one line per round and a JSON summary (median / min per shape); with AB_OUT=DIR also writes DIR/ab_<AB_TAG>.json.
Usage on the GPU box:  python tools/mfma_shape_ab.py   (profiles/r09_mfma_shape.md)"""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from typeagent_py_amd import _native

rows = int(os.environ.get("AB_ROWS", 10_000_000)); dim = 1536; nq = 1024; k = 32
rounds = int(os.environ.get("AB_ROUNDS", 6)); per = int(os.environ.get("AB_STEPS", 8))
g = torch.Generator(device="cuda").manual_seed(1234)
corpus = torch.empty((rows, dim), dtype=torch.float16, device="cuda")
for i in range(0, rows, 1 << 20):
    x = torch.randn((min(1 << 20, rows - i), dim), generator=g, device="cuda")
    corpus[i:i + x.shape[0]] = (x / x.norm(dim=1, keepdim=True)).half()
q = torch.randn((nq, dim), generator=g, device="cuda"); q = (q / q.norm(dim=1, keepdim=True)).contiguous()
eng = _native.Engine(0)
eng.set_corpus_tensor(corpus)
out = torch.empty((nq, k), dtype=torch.int64, device="cuda")
res = {16: [], 32: []}
ans = {}
def run(shape, n):
    eng.set_option("mfma_shape", shape)
    torch.cuda.synchronize(); eng.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        eng.search_device(q, k, 0.0, out_keys=out)
    eng.synchronize()
    return (time.perf_counter() - t) / n * 1e3
for s in (16, 32):
    run(s, 3)
    ans[s] = out.cpu().numpy().copy()
    print("shape", s, "ran", eng.get_option("last_mfma_shape"), flush=True)
print("bit-identical cfg3 answers:", bool(np.array_equal(ans[16], ans[32])), flush=True)
for r in range(rounds):
    for s in ((16, 32) if r % 2 == 0 else (32, 16)):
        res[s].append(run(s, per))
    print("round", r, {s: round(v[-1], 3) for s, v in res.items()}, flush=True)
summ = {s: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "all": [round(x, 3) for x in v]} for s, v in res.items()}
summ["speedup_median"] = summ[32]["median_ms"] / summ[16]["median_ms"]
print(json.dumps(summ), flush=True)
if os.environ.get("AB_OUT"):
    os.makedirs(os.environ["AB_OUT"], exist_ok=True)
    json.dump(summ, open(os.path.join(os.environ["AB_OUT"], f"ab_{os.environ.get('AB_TAG', 'x')}.json"), "w"), indent=1)
