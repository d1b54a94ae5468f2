"""CPU suite: the table of tests/test_gpu_large_k_planted.py (tests/large_k_planted_cases.py) reaches every branch of the large-k
selection and the sorted route it names, its planted formula is the oracle's arithmetic bit for bit, and its host model of the bucket map
and of `resolve` agrees with itself.

  * every name of `REQUIRED` is hit by a case, every case hits what it is in the table for, the names are unique, no corpus passes the
    size cap the module states, and the table's size is pinned so that a later edit cannot shrink it unseen;
  * `vo.scores_full` over the planted corpus equals the planted formula bit for bit for every query of every case (NaN rows as NaN),
    and `vo.check_topk_parity` accepts `expected` for every whole-corpus case with k <= rows;
  * the bucket map is monotone, `first_bits_at_least(j)` is the smallest bits whose bucket is >= j for every bucket count of the table,
    and after its last round the model's `above + inb` is a direct count over the planted keys, with `inb <= cap`."""

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import large_k_planted_cases as pc

IDS = [c.name for c in pc.CASES]


def test_table_is_what_the_suite_is_for():
    assert len(IDS) == len(set(IDS))
    assert len(pc.CASES) == 157
    assert {c.call for c in pc.CASES} == {"topk", "sorted", "messages"}
    assert pc.FAMILIES == ("counts", "need", "buckets", "depth", "last-subrange", "thresholds", "tails", "tiers", "batches", "sorted", "messages")
    assert all(c.family in pc.FAMILIES for c in pc.CASES) and max(sum(c.family == f for c in pc.CASES) for f in pc.FAMILIES) <= 40
    assert sum(c.call == "topk" for c in pc.CASES) == 86 and sum(c.call == "sorted" for c in pc.CASES) == 54 and sum(c.call == "messages" for c in pc.CASES) == 17
    for name in pc.CORPORA:
        p = pc.corpus_of(name)
        assert p.cos.shape[0] * p.dim <= pc.MAX_CORPUS_ELEMENTS, name
        assert p.dim * (2 if p.dtype == "fp16" else 4) % 16 == 0 or p.dim == 3, name
    assert set(pc.CLASS_CASES) <= set(IDS)
    by = {c.name: c for c in pc.CASES}
    assert [by[n].call for n in pc.CLASS_CASES] == ["topk", "topk", "sorted"]
    assert pc.expected_rounds(by[pc.CLASS_CASES[0]]) == 0 and pc.expected_rounds(by[pc.CLASS_CASES[1]]) == 4


def test_every_branch_has_a_case():
    hit = {}
    for c in pc.CASES:
        b = pc.branches(c)
        assert set(c.want) <= b, f"{c.name}: in the table for {sorted(set(c.want) - b)}, which it does not reach (it reaches {sorted(b)})"
        for name in b:
            hit.setdefault(name, []).append(c)
    assert pc.REQUIRED <= set(hit), f"no case for {sorted(pc.REQUIRED - set(hit))}"
    # the boundary bucket at the top, at bucket 0 and on both ends of an interior lane's walk, for every bucket count
    for nb in (256, 320, 1024, 4096):
        for spot in ("bucket-top", "bucket-0", "lane-first", "lane-last"):
            assert any(c.buckets == nb for c in hit[spot]), (nb, spot)
    # inb on both sides of both capacities; every depth under both; the tails and the chunk counts by their sizes
    for tag in ("inb-cap-1", "inb-cap", "inb-cap+1"):
        assert {c.cap for c in hit[tag]} >= {64, 1024}
    assert {c.cap for c in hit["refine-4"]} >= {64} and {c.cap for c in hit["refine-3"]} >= {1024} and {c.cap for c in hit["refine-1"]} >= {64, 1024}
    n_pos = lambda c: len(pc.position_scores(c, 0))
    assert {n_pos(c) for c in pc.CASES if c.name.startswith("tail-")} == {1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049}
    assert {n_pos(c) for c in hit["chunk-1"]} >= {2047, 2048} and {n_pos(c) for c in hit["chunk-2"]} >= {2049, 2559, 2560, 2561, 4096}
    assert {n_pos(c) for c in hit["chunk-3"]} >= {4097}
    assert pc.sorted_blocks(2049) == (2, 1280) and pc.sorted_blocks(2561) == (2, 1536) and pc.sorted_blocks(4097) == (3, 1536)
    assert pc.sel_blocks(2048, 1) == 1 and pc.sel_blocks(2049, 1) == 2 and pc.sel_blocks(130_000, 8) == 64
    # messages: the same selection over message ordinals, refined where the tie cases need it
    assert {c.call for c in hit["msg-tie-cap64"]} == {"messages"} and any(c.buckets == 4096 for c in hit["msg-zero-best"])
    assert {c.call for c in hit["last-subrange"]} == {"topk"}
    # batches: every size in both calls, fp16 among the batches of 8 and 9
    for nq in (1, 3, 8, 9):
        assert {c.call for c in hit[f"nq-{nq}"]} >= {"topk", "sorted"}
    assert {pc.corpus_of(c.corpus).dtype for c in hit["nq-9"]} == {"fp32", "fp16"}
    assert {pc.corpus_of(c.corpus).dtype for c in hit["tier-1"]} == {"fp32", "fp16"} and {pc.corpus_of(c.corpus).dtype for c in hit["tier-3"]} == {"fp32", "fp16"}


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_oracle_computes_the_planted_formula(case):
    v = pc.vectors(case)
    qs = pc.queries(case)
    whole = case.call != "messages"
    for qi in range(case.nq):
        with np.errstate(invalid="ignore"):
            ref = np.asarray(vo.scores_full(v, qs[qi]), dtype=np.float32)
        want = pc.row_scores(case, qi)
        assert np.array_equal(np.isnan(ref), np.isnan(want))
        ok = ~np.isnan(want)
        assert np.array_equal(ref[ok].view(np.uint32), want[ok].view(np.uint32)), f"{case.name} q{qi}"
        k = pc.effective_k(case, len(want))
        if whole and k <= len(want):
            ords, bits = pc.expected(case, qi)
            with np.errstate(invalid="ignore"):
                vo.check_topk_parity(ref, ords.tolist(), bits.view(np.float32).tolist(), k, np.float32(case.thr[qi]))


@pytest.mark.parametrize("nb", sorted({c.buckets for c in pc.CASES}))
@pytest.mark.parametrize("thr", [0.0, 0.5, 0.3, 0.999, 1.0, -0.2])
def test_bucket_map_is_monotone_and_the_bisection_finds_its_edges(nb, thr):
    lo, scale = pc.bucket_params(thr, nb)
    rng = np.random.default_rng(nb)
    bits = np.unique(np.concatenate([np.linspace(0, pc.ONE_BITS, 200_001).astype(np.uint32), rng.integers(0, pc.ONE_BITS + 1, 100_000).astype(np.uint32),
                                     np.array([0, 1, pc.HALF_BITS, pc.ONE_BITS - 1, pc.ONE_BITS], dtype=np.uint32)]))
    b = pc.bucket_map(bits.view(np.float32), lo, scale, nb)
    assert np.all(np.diff(b) >= 0) and b.min() >= 0 and b.max() <= nb - 1
    if scale == 0:
        assert b.max() == 0
    for j in sorted({0, 1, nb // 3, nb // 2, nb - 2, nb - 1, nb, *rng.integers(0, nb, 12).tolist()}):
        a = pc.first_bits_at_least(j, lo, scale, nb)
        at = lambda x: int(pc.bucket_map(np.array([x], dtype=np.uint32).view(np.float32), lo, scale, nb)[0])
        if a <= pc.ONE_BITS:
            assert at(a) >= j
        else:
            assert a == pc.ONE_BITS + 1 and at(pc.ONE_BITS) < j
        assert a == 0 or at(a - 1) < j
    assert pc.first_bits_at_least(0, lo, scale, nb) == 0 and pc.first_bits_at_least(nb, lo, scale, nb) == pc.ONE_BITS + 1


@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_model_agrees_with_a_direct_count(case):
    for qi in range(case.nq):
        m = pc.model(case, qi)
        s = pc.position_scores(case, qi)
        pos = pc.passing(s, case.thr[qi])
        assert m.empty == (len(pos) == 0)
        if m.empty:
            assert pc.expected(case, qi)[0].size == 0
            continue
        keys = pc.row_keys(s, pos)
        assert m.need == min(pc.effective_k(case, len(s)), len(pos)) and m.total == len(pos)
        assert m.above == int(np.sum(keys > np.uint64(m.kb))) and m.inb == int(np.sum((keys >= np.uint64(m.ka)) & (keys <= np.uint64(m.kb))))
        assert m.above < m.need <= m.above + m.inb  # the rank-need key lies inside the range
        assert m.rounds <= pc.rounds_enqueued(case, len(s))
        if pc.rounds_enqueued(case, len(s)):
            assert m.inb <= case.cap, f"{case.name} q{qi}: {m.inb} keys after {m.rounds} rounds"
        ords, bits = pc.expected(case, qi)
        assert len(ords) == m.need and np.all(np.diff(bits.astype(np.int64)) <= 0)
        assert int(np.sort(keys)[::-1][m.need - 1]) >= m.ka


def test_refine_rounds_table():
    assert [pc.topk_refine_rounds(n, cap) for n, cap in ((64, 64), (65, 64), (1025, 1024), (16384, 16384), (16385, 16384))] == [0, 5, 5, 0, 5]
