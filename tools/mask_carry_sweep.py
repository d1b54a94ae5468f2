"""Row masks carried through row edits: `remove_rows(carry=)` / `insert_rows(carry=)` (tavb_mask_remap on the packed masks) against the same
edit without handles and against the only way there was to keep scopes alive before -- the edit, then the caller's host bool arrays
through np.delete / np.insert and `row_mask` again, once per mask.  A device-only fp16 corpus; masks of 1 / 10 / 50 %; one row, a block
of 1 % and a random 1 % removed and put back (the insertion re-opens the removed positions, so the index keeps its size); 1 and 8
handles.  The three legs are interleaved in one process, 3 rounds x 3 calls each; a cell reports the median of its 9 calls and, for the
rebuild leg, the spread of its rounds' medians -- the margin the comparison has.  Prints a markdown table
(profiles/r24_mask_carry.md) and one JSON line per cell.

    python tools/mask_carry_sweep.py [--rows 1000000] [--dim 1536] [--rounds 3] [--calls 3]
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

EDITS = ("one row", "block of 1 %", "random 1 %")
LEGS = ("carry", "plain", "rebuild")


def edited(kind: str, rows: int) -> np.ndarray:
    if kind == "one row":
        return np.array([rows // 2])
    if kind == "block of 1 %":
        return np.arange(rows // 2, rows // 2 + rows // 100)
    return np.sort(np.random.default_rng(24).choice(rows, size=rows // 100, replace=False))


def ms(fn) -> float:
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()
    rows, dim = args.rows, args.dim
    rng = np.random.default_rng(1)
    v = rng.standard_normal((rows, dim), dtype=np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype="fp16", keep_host_copy=False)
    vb.add_embeddings(None, v)
    vb.fuzzy_lookup_embedding(v[0], 10, 0.0)
    assert vb._device_only is not None
    print("| mask density | handles | edit | remove: carry ms | no handles ms | + rebuild ms | rebuild rounds ms | insert: carry ms | no handles ms | + rebuild ms | rebuild rounds ms |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for pct in (1, 10, 50):
        for n_masks in (1, 8):
            for kind in EDITS:
                idx = edited(kind, rows)
                at = idx - np.arange(len(idx))  # the same positions opened again
                new = v[idx]
                bools = [np.random.default_rng(100 * pct + i).random(rows) * 100 < pct for i in range(n_masks)]
                times = {(leg, op): [[] for _ in range(args.rounds)] for leg in LEGS for op in ("remove", "insert")}
                for rnd in range(args.rounds):
                    for leg in LEGS:
                        handles = [vb.row_mask(b) for b in bools]  # (not timed: every leg starts from valid handles)
                        for _ in range(args.calls):
                            if leg == "carry":
                                t_rm = ms(lambda: vb.remove_rows(idx, carry=handles))
                                t_in = ms(lambda: vb.insert_rows(at, new, carry=handles))
                                bools = [np.insert(np.delete(b, idx), at, False) for b in bools]
                            elif leg == "plain":
                                t_rm = ms(lambda: vb.remove_rows(idx))
                                t_in = ms(lambda: vb.insert_rows(at, new))
                                bools = [np.insert(np.delete(b, idx), at, False) for b in bools]
                            else:
                                def remove_and_rebuild():
                                    nonlocal bools, handles
                                    vb.remove_rows(idx)
                                    bools = [np.delete(b, idx) for b in bools]
                                    handles = [vb.row_mask(b) for b in bools]

                                def insert_and_rebuild():
                                    nonlocal bools, handles
                                    vb.insert_rows(at, new)
                                    bools = [np.insert(b, at, False) for b in bools]
                                    handles = [vb.row_mask(b) for b in bools]

                                t_rm, t_in = ms(remove_and_rebuild), ms(insert_and_rebuild)
                            times[(leg, "remove")][rnd].append(t_rm)
                            times[(leg, "insert")][rnd].append(t_in)
                        if leg != "plain":  # the handles followed the edits: they name what the host bools name
                            assert len(vb) == rows and all(h.count == int(b.sum()) for h, b in zip(handles, bools))
                cell = {"rows": rows, "dim": dim, "mask_pct": pct, "handles": n_masks, "edit": kind, "edited_rows": int(len(idx))}
                out = [f"{pct} %", str(n_masks), kind]
                for op in ("remove", "insert"):
                    for leg in LEGS:
                        per_round = [float(np.median(r)) for r in times[(leg, op)]]
                        cell[f"{op}_{leg}_ms"] = float(np.median(np.concatenate(times[(leg, op)])))
                        cell[f"{op}_{leg}_rounds_ms"] = per_round
                        out.append(f"{cell[f'{op}_{leg}_ms']:.2f}")
                    r = cell[f"{op}_rebuild_rounds_ms"]
                    out.append(f"{min(r):.2f} .. {max(r):.2f}")
                print("| " + " | ".join(out) + " |", flush=True)
                print("JSON " + json.dumps(cell), flush=True)


if __name__ == "__main__":
    main()
