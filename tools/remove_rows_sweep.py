"""Removing rows: `VectorBase.remove_rows` (the corpus compacted on the device, tavb_compact_rows) against the only route there was before
it -- np.delete of the host matrix, `deserialize()` of the result and the whole-corpus upload of the next lookup; for a device-only
corpus `serialize()` first -- interleaved on the same box.  Per cell: the removal, then the first lookup after it (1 query; on fp32 also
64 queries, so that the refresh of the fp16 shadow is in it), and the bytes the compaction moves against the bytes from the first removed
row to the end.  Prints a markdown table (profiles/r18_remove_rows.md) and one JSON line per cell.

    python tools/remove_rows_sweep.py [--rows 1000000] [--dim 1536] [--dtypes fp16,fp32] [--skip-parent]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.fakes import NullModel  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase  # noqa: E402


def removed(kind: str, rows: int) -> np.ndarray:
    rng = np.random.default_rng(18)
    if kind == "first":
        return np.array([0])
    if kind == "middle":
        return np.array([rows // 2])
    if kind == "last":
        return np.array([rows - 1])
    if kind == "random 1 %":
        return np.sort(rng.choice(rows, size=rows // 100, replace=False))
    if kind == "random 50 %":
        return np.sort(rng.choice(rows, size=rows // 2, replace=False))
    return np.arange(rows // 4, rows // 4 + rows // 2)  # a contiguous 50 %


KINDS = ("first", "middle", "last", "random 1 %", "random 50 %", "contiguous 50 %")


def ms(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def moved_bytes(idx: np.ndarray, rows: int, row_bytes: int) -> tuple[int, int]:
    """(bytes the in-place compaction reads and writes, bytes from the first removed row to the end)"""
    start = int(idx[0]) // 64 * 64
    kept_after = (rows - start) - int(np.count_nonzero(idx >= start))
    return ((rows - start) + 3 * kept_after) * row_bytes, (rows - int(idx[0])) * row_bytes


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--skip-parent", action="store_true")
    args = ap.parse_args()
    rows, dim = args.rows, args.dim
    rng = np.random.default_rng(1)
    v = rng.standard_normal((rows, dim), dtype=np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    qs = rng.standard_normal((64, dim), dtype=np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    settings = TextEmbeddingIndexSettings(NullModel())
    print("| dtype | corpus | removed | remove_rows ms | next lookup ms (1 q) | (64 q) | parent: np.delete + deserialize ms | parent next lookup ms (1 q) | (64 q) | "
          "moved / behind first removed (MB) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for dtype in args.dtypes.split(","):
        row_bytes = dim * (2 if dtype == "fp16" else 4)
        for host in (True, False):
            for kind in KINDS:
                idx = removed(kind, rows)
                cell = {"dtype": dtype, "corpus": "mirror of a host matrix" if host else "device only", "removed": kind, "rows": rows, "dim": dim}

                def build():
                    vb = VectorBase(settings, corpus_dtype=dtype, keep_host_copy=host)
                    vb.add_embeddings(None, v)
                    vb.fuzzy_lookup_embedding(qs[0], 10, 0.0)
                    if dtype == "fp32":
                        vb.fuzzy_lookup_embeddings(qs, 10, 0.0)  # the shadow and the row-norm maxima exist
                    return vb

                vb = build()
                cell["remove_ms"] = ms(lambda: vb.remove_rows(idx))
                cell["lookup1_ms"] = ms(lambda: vb.fuzzy_lookup_embedding(qs[0], 10, 0.0))
                cell["lookup64_ms"] = ms(lambda: vb.fuzzy_lookup_embeddings(qs, 10, 0.0)) if dtype == "fp32" else None
                want = [r.item for r in vb.fuzzy_lookup_embedding(qs[1], 10, 0.0)]
                del vb
                if not args.skip_parent:
                    vb = build()

                    def parent():
                        vb.deserialize(np.delete(np.asarray(vb.serialize()), idx, axis=0))

                    cell["parent_remove_ms"] = ms(parent)
                    cell["parent_lookup1_ms"] = ms(lambda: vb.fuzzy_lookup_embedding(qs[0], 10, 0.0))
                    cell["parent_lookup64_ms"] = ms(lambda: vb.fuzzy_lookup_embeddings(qs, 10, 0.0)) if dtype == "fp32" else None
                    assert [r.item for r in vb.fuzzy_lookup_embedding(qs[1], 10, 0.0)] == want, "the two routes disagree"
                    del vb
                cell["moved_bytes"], cell["behind_first_bytes"] = moved_bytes(idx, rows, row_bytes)
                f = lambda x: "-" if x is None else f"{x:.2f}"
                print(f"| {dtype} | {cell['corpus']} | {kind} | {f(cell['remove_ms'])} | {f(cell['lookup1_ms'])} | {f(cell['lookup64_ms'])} | "
                      f"{f(cell.get('parent_remove_ms'))} | {f(cell.get('parent_lookup1_ms'))} | {f(cell.get('parent_lookup64_ms'))} | "
                      f"{cell['moved_bytes'] / 1e6:.0f} / {cell['behind_first_bytes'] / 1e6:.0f} |", flush=True)
                print("JSON " + json.dumps(cell), flush=True)


if __name__ == "__main__":
    main()
