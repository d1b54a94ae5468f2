"""Inserting and overwriting rows: `VectorBase.insert_rows` / `set_rows` (the corpus expanded on the device, tavb_expand_rows, and only
the new rows sent, tavb_scatter_rows) against the only route there was before them -- `vb._vectors = np.insert(...)`, resp. an
assignment into the host matrix, and the whole-corpus upload of the next lookup; for a device-only corpus `serialize()` first --
interleaved in one process on the same box, `--repeats` times per cell.  Per cell and leg: the edit, then the first batched lookup after
it (64 queries, so that on fp32 the refresh of the fp16 shadow is in it); median and [min, max].  Prints a markdown table
(profiles/r19_insert_rows.md) and one JSON line per cell.

    python tools/insert_rows_sweep.py [--rows 1000000] [--dim 1536] [--dtypes fp16,fp32] [--repeats 3] [--skip-parent]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.fakes import NullModel  # noqa: E402
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase  # noqa: E402

INSERTS = ("insert 1 at front", "insert 1 in middle", "insert 1 at end", "insert block of 1 %", "insert random 1 %", "insert random 50 %")
WRITES = ("set 10 rows", "set random 1 %")


def edit(kind: str, rows: int):
    """(at or which, how many new rows)"""
    rng = np.random.default_rng(19)
    if kind == "insert 1 at front":
        return 0, 1
    if kind == "insert 1 in middle":
        return rows // 2, 1
    if kind == "insert 1 at end":
        return rows, 1
    if kind == "insert block of 1 %":
        return rows // 2, rows // 100
    if kind == "insert random 1 %":
        return np.sort(rng.integers(0, rows + 1, size=rows // 100)), rows // 100
    if kind == "insert random 50 %":
        return np.sort(rng.integers(0, rows + 1, size=rows // 2)), rows // 2
    m = 10 if kind == "set 10 rows" else rows // 100
    return np.sort(rng.choice(rows, size=m, replace=False)), m


def ms(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def spread(xs) -> str:
    return "-" if not xs else f"{statistics.median(xs):.2f} [{min(xs):.2f}, {max(xs):.2f}]"


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--dtypes", default="fp16,fp32")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kinds", default=",".join(INSERTS + WRITES))
    ap.add_argument("--skip-parent", action="store_true")
    args = ap.parse_args()
    rows, dim = args.rows, args.dim
    rng = np.random.default_rng(1)
    v = rng.standard_normal((rows + rows // 2, dim), dtype=np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    v, fresh_rows = v[:rows], v[rows:]  # the corpus; the rows that come
    qs = rng.standard_normal((64, dim), dtype=np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    settings = TextEmbeddingIndexSettings(NullModel())
    print("| dtype | corpus | edit | new route: edit ms | new route: next 64-query lookup ms | parent route: edit ms | parent route: next 64-query lookup ms |")
    print("|---|---|---|---|---|---|---|")
    for dtype in args.dtypes.split(","):
        for host in (False, True):
            for kind in args.kinds.split(","):
                where, m = edit(kind, rows)
                new = fresh_rows[:m]
                cell = {"dtype": dtype, "corpus": "mirror of a host matrix" if host else "device only", "edit": kind, "rows": rows, "dim": dim,
                        "edit_ms": [], "lookup_ms": [], "parent_edit_ms": [], "parent_lookup_ms": []}

                def build():
                    vb = VectorBase(settings, corpus_dtype=dtype, keep_host_copy=host)
                    vb.add_embeddings(None, v)
                    vb.fuzzy_lookup_embedding(qs[0], 10, 0.0)
                    vb.fuzzy_lookup_embeddings(qs, 10, 0.0)  # the row-norm maxima (fp32: and the shadow) exist
                    return vb

                for _ in range(args.repeats):  # the two legs take turns
                    vb = build()
                    if kind.startswith("insert"):
                        cell["edit_ms"].append(ms(lambda: vb.insert_rows(where, new)))
                    else:
                        cell["edit_ms"].append(ms(lambda: vb.set_rows(where, new)))
                    cell["lookup_ms"].append(ms(lambda: vb.fuzzy_lookup_embeddings(qs, 10, 0.0)))
                    want = [r.item for r in vb.fuzzy_lookup_embedding(qs[1], 10, 0.0)]
                    del vb
                    if args.skip_parent:
                        continue
                    vb = build()

                    def parent():
                        if kind.startswith("insert"):
                            vb._vectors = np.insert(np.asarray(vb.serialize()), where, new, axis=0)
                        else:
                            vb._vectors[where] = new

                    cell["parent_edit_ms"].append(ms(parent))
                    cell["parent_lookup_ms"].append(ms(lambda: vb.fuzzy_lookup_embeddings(qs, 10, 0.0)))
                    assert [r.item for r in vb.fuzzy_lookup_embedding(qs[1], 10, 0.0)] == want, "the two routes disagree"
                    del vb
                print(f"| {dtype} | {cell['corpus']} | {kind} | {spread(cell['edit_ms'])} | {spread(cell['lookup_ms'])} | {spread(cell['parent_edit_ms'])} | "
                      f"{spread(cell['parent_lookup_ms'])} |", flush=True)
                print("JSON " + json.dumps(cell), flush=True)


if __name__ == "__main__":
    main()
