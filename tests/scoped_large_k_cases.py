"""TEST INFRASTRUCTURE -- the case table of scoped batches beyond the fused selection (tavb_search_scoped_topk for max_hits 257 .. 16384,
tavb_search_scoped_sorted for max_hits 0 and beyond 16384), shared by tests/test_gpu_scoped_large_k.py (the device) and
tests/test_scoped_large_k_host.py (its CPU twin, which pins the table's own claims).

The scope families, the corpora and the threshold cycle are those of tests/scoped_batch_cases.py, imported, not copied.  A pass of these
routes is eight queries at every max_hits (the bits of a membership byte), so the batches are a partial pass (1, 2), a full pass (8), a
trailing pass of one (9) and three passes (17).  The row counts put max_hits on both sides of a scope's size: 257 rows are fewer than
every max_hits but 257 itself, 20000 rows are more than 16385.  Corpora, row counts, thresholds and the form of the scopes rotate through
the cases so that each of them meets every value of the others and of (batch, max_hits, family).

`score_pass_twin` restates the scoped score pass in numpy."""

from __future__ import annotations

import numpy as np

from tests import scoped_batch_cases as sc
from tests.scoped_batch_cases import CORPORA, FAMILIES, THR_CYCLE, Case, case_scopes, case_thresholds, expect_native, member_bytes  # noqa: F401

ROWS = (257, 1000, 4099, 20000)
BATCHES = (1, 2, 8, 9, 17)
MAX_HITS = (0, 257, 300, 1000, 4096, 16384, 16385)
MAX_ROWS = max(ROWS)
MAX_QUERIES = max(BATCHES)
PER_PASS = 8

SCORE_NONE = 0xFFFFFFFF  # kScoreNone: the score-array slot of a row that did not pass, or that the query's scope does not hold


def _cases() -> tuple[Case, ...]:
    out = []
    i = 0
    for k in MAX_HITS:
        for nq in BATCHES:
            for family in FAMILIES:
                # i runs over 350 cases; the strides are those of the scoped table (corpus slips every 7 cases, the others every 10)
                out.append(Case(CORPORA[(i + i // 7) % len(CORPORA)], ROWS[(i + i // 10) % len(ROWS)], nq, k, family,
                                "per_query" if (i + i // 10) % 3 == 0 else "uniform", (i + i // 10) % 5 != 0))
                i += 1
    return tuple(out)


CASES = _cases()
ORDINAL_BASE = sc.ORDINAL_BASE
# the adopted-corpus case of the scoped table, at a max_hits of each route
ADOPTED = tuple(Case(sc.ADOPTED.corpus, sc.ADOPTED.rows, sc.ADOPTED.nq, k, sc.ADOPTED.family, sc.ADOPTED.thresholds, True) for k in (300, 0))


def route_of(max_hits: int) -> int:
    """What "masked_route" reports after a scoped batch at this max_hits: 7 = the large-k route, 8 = the sorted route."""
    return 7 if 257 <= max_hits <= 16384 else 8


def passes(nq: int) -> list[int]:
    """The queries of every pass of a scoped large-k or sorted batch."""
    return [min(PER_PASS, nq - q0) for q0 in range(0, nq, PER_PASS)]


def score_pass_twin(scores: np.ndarray, member: np.ndarray, min_scores, bit0: int = 0):
    """The scoped score pass in numpy.  scores: float32 [nq, n_pos], the single-query pass' score of every union position; member: uint8
    [n_pos]; query j is member bit bit0 + j -> (uint32 [nq, n_pos]: the score's bits where the bit is set and the score passes
    min_scores[j], SCORE_NONE elsewhere; the number of such positions per query: what the query's histogram sums to)."""
    nq, n_pos = scores.shape
    out = np.full((nq, n_pos), SCORE_NONE, dtype=np.uint32)
    counts = []
    for j in range(nq):
        ok = ((member >> (bit0 + j)) & 1).astype(bool) & (scores[j] >= np.float32(min_scores[j]))
        out[j, ok] = scores[j, ok].view(np.uint32)
        counts.append(int(ok.sum()))
    return out, counts
