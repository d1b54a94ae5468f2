"""CPU suite: the table of tests/test_gpu_helper_kernels.py (tests/helper_kernel_cases.py) holds a case for every branch of the helper
kernels of csrc/tavb_misc.hip, and its numpy references are right where there is something to check them against.

  * the classifiers restate the launch code; every class they name has a case, and the table's size is pinned so that a later edit cannot
    shrink coverage unseen;
  * the host twin of the merge kernel (`_native.merge_keys`) equals the sort of the union on every merge case;
  * `vo.l2_normalize_rows` itself passes the assertions the kernel has to pass -- the special rows, the float64 bound and the IEEE
    quotient -- and a reciprocal-multiply does not;
  * the remap reference equals a Python loop; the conversion reference (numpy's float16 cast) rounds the named values as IEEE says;
  * the re-rank inputs leave no doubt about the order of the hits, and the oracle's answers have the shapes the cases are there for."""

import numpy as np
import pytest

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests import helper_kernel_cases as hc
from typeagent_py_amd import _native


def test_table_holds_what_the_suite_is_for():
    assert (len(hc.MERGE_CASES), len(hc.NORM_CASES), len(hc.CONV_CASES), len(hc.UPLOAD_CASES), len(hc.REMAP_CASES), len(hc.RERANK_CASES)) == (90, 25, 8, 4, 3, 35)
    for cases in (hc.MERGE_CASES, hc.NORM_CASES, hc.CONV_CASES, hc.UPLOAD_CASES, hc.REMAP_CASES, hc.RERANK_CASES):
        assert len({c.name for c in cases}) == len(cases)
    # merge: every list count, every k, all nine k at 3, 8 and 17 lists, both query counts, every fill
    assert sorted({c.n_lists for c in hc.MERGE_CASES}) == list(hc.MERGE_COUNTS) and sorted({c.k for c in hc.MERGE_CASES}) == list(hc.MERGE_KS)
    for n in (3, 8, 17):
        assert sorted({c.k for c in hc.MERGE_CASES if c.n_lists == n and c.fill in ("full", "ragged")}) == list(hc.MERGE_KS)
    assert {c.nq for c in hc.MERGE_CASES} == {1, 3} and {c.fill for c in hc.MERGE_CASES} == set(hc.MERGE_FILLS)
    # normalise: every width aligned, every vector width through the unaligned view as well, the two tall cases
    assert sorted(c.dim for c in hc.NORM_CASES if c.offset == 0 and c.rows <= 70) == sorted(hc.NORM_VECTOR_WIDTHS + hc.NORM_SCALAR_WIDTHS)
    assert sorted(c.dim for c in hc.NORM_CASES if c.offset) == sorted(hc.NORM_VECTOR_WIDTHS)
    assert all(7 <= c.rows <= 70 for c in hc.NORM_CASES if c.rows < 8000)
    assert {(c.rows, c.dim) for c in hc.NORM_CASES if c.rows >= 8000} == {(8200, 8), (8195, 1540)}
    # convert, upload, remap
    assert hc.CONV_BIG == 2048 * 256 * 8 + 8 * 300 + 5
    assert sorted(c.count for c in hc.CONV_CASES if not c.offset) == [1, 7, 8, 9, hc.CONV_BIG] and hc.CONV_BIG in {c.count for c in hc.CONV_CASES if c.offset}
    assert {(c.rows, c.dim, c.parts, c.dtype) for c in hc.UPLOAD_CASES} == {(r, d, p, t) for r, d, p in ((2500, 4099, (2500,)), (300, 33, (1, 10, 289)))
                                                                           for t in ("fp16", "fp32")}
    assert {(c.count, c.map_len) for c in hc.REMAP_CASES} >= {(300_000, 1000)} and {c.map_len for c in hc.REMAP_CASES} >= {1} and {c.count for c in hc.REMAP_CASES} >= {1}
    # re-rank: every map with every accept collection, and the subset form over every map
    maps = {("one", 256), ("own", 256), ("own", 255), ("none", 256), ("blocks", 1), ("blocks", 37), ("blocks", 256)}
    for accept in ("none", "even", "long-head", "long-tail"):
        assert {(c.rows_map, c.max_matches) for c in hc.RERANK_CASES if c.form == "embedding" and c.accept == accept} == maps
    assert {(c.rows_map, c.max_matches) for c in hc.RERANK_CASES if c.form == "subset"} == maps
    assert hc.ACCEPT_LONG > 1024 * 256 and hc.REMAP_CASES[0].count > hc.REMAP_GRID_THREADS


def test_every_branch_has_a_case():
    merge = {}
    for c in hc.MERGE_CASES:
        for b in hc.merge_branches(c.n_lists, c.k):
            merge.setdefault(b, []).append(c)
    assert set(merge) >= {"kpl1", "kpl4", "tail", "tail-rounds", "four-per-round", "kpl4-rounds", "odd", "block-merge", "waves1", "waves2", "waves4", "waves8", "waves16"}
    # what the issue names: the four-keys-per-lane form, odd counts, more lists than waves, 49 lists and more, short and empty lists, the failure key
    assert {c.k for c in merge["kpl4"]} == {65, 128, 200, 255, 256} and {c.k for c in merge["kpl1"]} == {1, 2, 63, 64}
    assert {c.n_lists for c in merge["four-per-round"]} == {49, 64, 65, 100} and {c.n_lists for c in merge["tail-rounds"]} >= {17, 33, 48}
    assert {c.n_lists for c in merge["kpl4-rounds"]} >= {17, 33, 48, 49, 64, 65, 100}
    # 49 lists on 16 waves: wave 0 folds lists 0, 16, 32, 48 in one round, every other wave its three in the tail loop
    assert hc.merge_branches(49, 64) >= {"four-per-round", "tail-rounds"} and "tail" not in hc.merge_branches(64, 64)
    for fill in ("failed", "ties", "high", "one"):
        assert {b for c in hc.MERGE_CASES if c.fill == fill for b in hc.merge_branches(c.n_lists, c.k)} >= {"kpl1", "kpl4"}, fill

    norm = {}
    for c in hc.NORM_CASES:
        for b in hc.norm_branch(c):
            norm.setdefault(b, []).append(c)
    assert set(norm) == {"in-registers-6", "in-registers-16", "vector-streamed", "scalar", "unaligned-fallback", "grid-stride"}
    assert sorted(c.dim for c in norm["in-registers-6"] if c.rows <= 70) == [4, 1532, 1536]
    assert sorted(c.dim for c in norm["in-registers-16"] if c.rows <= 70) == [1540, 3072, 4092, 4096]
    assert sorted(c.dim for c in norm["vector-streamed"]) == [4100, 4104, 6144] and sorted(c.dim for c in norm["scalar"]) == [1537, 3073, 4098]
    assert {tuple(sorted(hc.norm_branch(c))) for c in norm["grid-stride"]} == {("grid-stride", "in-registers-6"), ("grid-stride", "in-registers-16")}

    conv = {}
    for c in hc.CONV_CASES:
        for b in hc.conv_branches(c):
            conv.setdefault(b, []).append(c.name)
    assert set(conv) == {"vector", "tail", "unaligned", "grid-stride", "unaligned-grid-stride"}
    assert hc.conv_branches(hc.CONV_CASES[0]) == {"vector", "tail", "grid-stride"}
    assert hc.conv_branches(hc.ConvCase("x", 7)) == {"tail"} and hc.conv_branches(hc.ConvCase("x", 8)) == {"vector"}

    up = {c.name: hc.upload_chunks(c) for c in hc.UPLOAD_CASES}
    assert up["upload-2500x4099-fp16"] == [(0, 1023, 0), (1023, 1023, 10), (2046, 454, 4)]  # three staging chunks, the second and third unaligned
    assert up["upload-300x33-fp16"] == [(0, 1, 0), (1, 10, 2), (11, 289, 6)]  # appends at odd rows
    assert [c[:2] for c in up["upload-2500x4099-fp32"]] == [c[:2] for c in up["upload-2500x4099-fp16"]]


# ---- merge -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.MERGE_CASES, ids=[c.name for c in hc.MERGE_CASES])
def test_host_merge_equals_the_sort_of_the_union(case):
    lists = hc.merge_lists(case)
    assert lists.shape == (case.n_lists, case.nq, case.k)
    for q in range(case.nq):  # the inputs are what the kernel is promised: sorted, zero-padded, unique within a query
        for l in range(case.n_lists):
            assert (lists[l, q, :-1] >= lists[l, q, 1:]).all()
        live = lists[:, q, :][(lists[:, q, :] != 0) & (lists[:, q, :] != hc.FAILED)]
        assert len(np.unique(live)) == len(live)
    want = hc.merged_by_sort(lists)
    np.testing.assert_array_equal(_native.merge_keys(lists), want)
    if case.fill == "ragged":
        assert (lists[:, :, 0] == 0).any() and (case.nq == 1 or (lists[:, case.nq - 1] == 0).all())
    if case.fill == "one":
        assert ((lists[:, :, 0] != 0).sum(axis=0) == 1).all()
    if case.fill == "ties":
        assert len(np.unique(lists >> np.uint64(32))) == 2
    if case.fill == "high":
        assert ((lists & hc.U32)[lists != 0] <= np.uint64(1 + 3 * case.n_lists * case.k)).all()  # 0xFFFFFFFF - ordinal: ordinals from 2^32 - 2 down
    if case.fill == "failed":
        assert want[1, 0] == hc.FAILED and (want[[0, 2]] != hc.FAILED).all()
        with pytest.raises(_native.TavbError, match="a rank of the collective lookup failed"):
            _native.decode_keys(want)
        _native.decode_keys(want[[0, 2]])


# ---- normalise -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.NORM_CASES, ids=[c.name for c in hc.NORM_CASES])
def test_the_oracle_passes_the_normalise_assertions(case):
    x = hc.norm_input(case)
    assert not x[0].any() and np.isnan(x[1]).sum() == 1 and np.isposinf(x[2]).sum() == 1 and (np.abs(x[3]) == np.float32(1e20)).sum() >= 2
    assert (x[4] != 0).sum() == 1 and np.isfinite(x[hc.NORM_SPECIAL_ROWS:]).all() and len(x) >= hc.NORM_SPECIAL_ROWS + 2
    with np.errstate(over="ignore", invalid="ignore"):
        y = vo.l2_normalize_rows(x)
    # what numpy makes of the special rows: a NaN norm divides by 1, an inf norm leaves (+-)0 and inf / inf = NaN
    assert not y[0].any() and np.array_equal(y[1], x[1], equal_nan=True) and np.isnan(y[2]).sum() == 1 and (y[2][~np.isnan(y[2])] == 0).all()
    assert (y[3] == 0).all() and np.signbit(y[3][case.dim - 1]) and (y[4] != 0).sum() == 1 and y[4].min() == -1.0
    fig = hc.norm_check(case, x, y, y)
    assert fig["worst_units"] <= 3.0  # one rounding of the norm, one of the quotient, and a pairwise sum: far inside the kernel's worst case


def test_a_reciprocal_multiply_fails_the_ieee_assertion():
    """... and a wrong element fails both: the assertions are not vacuous"""
    case = next(c for c in hc.NORM_CASES if c.name == "norm-d3072")
    x = hc.norm_input(case)
    with np.errstate(over="ignore", invalid="ignore"):
        oracle = vo.l2_normalize_rows(x)
    norms = np.linalg.norm(x[hc.NORM_SPECIAL_ROWS:], axis=1, keepdims=True).astype(np.float32)
    y = oracle.copy()
    y[hc.NORM_SPECIAL_ROWS:] = x[hc.NORM_SPECIAL_ROWS:] * (np.float32(1.0) / norms)
    with pytest.raises(AssertionError, match="no IEEE float32 quotient"):
        hc.norm_check(case, x, y, oracle)
    y = oracle.copy()
    y[hc.NORM_SPECIAL_ROWS + 1, 17] *= np.float32(1 + 2.0**-17)
    with pytest.raises(AssertionError, match="units of 2\\^-24"):
        hc.norm_check(case, x, y, oracle)
    y = oracle.copy()
    y[3, 0] = -0.0  # the sign of a zero in a special row
    with pytest.raises(AssertionError, match="special rows differ"):
        hc.norm_check(case, x, y, oracle)
    assert hc.norm_bound_units(3072) == 29.0 and hc.norm_bound_units(4) == 5.5 and hc.norm_bound_units(4100) == 37.5


# ---- convert ---------------------------------------------------------------------------------------------------------------------------

def test_the_conversion_reference_rounds_to_nearest_even():
    h = lambda v: np.float32(v).astype(np.float16)
    with np.errstate(over="ignore"):
        assert h(65519.99) == 65504 and np.isposinf(h(65520.0)) and np.isneginf(h(-65520.0)) and h(65504.0) == 65504
    assert h(2.0**-24) == 2.0**-24 and h(2.0**-25) == 0 and h(1.5 * 2.0**-25) == 2.0**-24 and h(3 * 2.0**-25) == 2.0**-23
    assert np.signbit(h(-(2.0**-25))) and h(-(2.0**-25)) == 0 and float(h(6.0e-5)) == round(6.0e-5 * 2**24) * 2.0**-24
    for j in range(8):  # a tie between 1 + j * 2^-10 and 1 + (j + 1) * 2^-10 goes to the even one
        assert float(h(1 + (2 * j + 1) * 2.0**-11)) == 1 + (j + j % 2) * 2.0**-10
    for case in hc.CONV_CASES:
        x = hc.conv_input(case)
        assert x.shape == (case.count,)
        if case.count > 100:  # every special value at the head, behind the grid's first pass and in the scalar tail
            s = len(hc.CONV_SPECIALS)
            edge = hc.CONV_GRID_THREADS * 8
            for at in (0, edge - 3):
                assert np.array_equal(x[at : at + s].view(np.uint32), hc.CONV_SPECIALS.view(np.uint32))
            assert case.count % 8 == 5
            assert np.array_equal(x[-5:].view(np.uint32), hc.CONV_SPECIALS[::-1][-5:].view(np.uint32))
        with np.errstate(over="ignore"):
            hc.conv_check(x, x.astype(np.float16), case.name)
    seen = np.concatenate([hc.conv_input(c) for c in hc.CONV_CASES if c.count < 100])
    assert np.isin(hc.CONV_SPECIALS[~np.isnan(hc.CONV_SPECIALS)], seen).all()  # the short counts together carry every special value too


# ---- remap -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.REMAP_CASES, ids=[c.name for c in hc.REMAP_CASES])
def test_the_remap_reference_equals_a_python_loop(case):
    keys, m = hc.remap_input(case)
    assert keys.shape == (case.count,) and m.shape == (case.map_len,) and m.dtype == np.int32
    want = hc.remap_reference(keys, m)
    for i in range(min(case.count, 3000)):
        key = int(keys[i])
        if key == 0:
            assert want[i] == 0
            continue
        pos = 0xFFFFFFFF - (key & 0xFFFFFFFF)
        to = int(m[pos]) if pos < case.map_len else 0xFFFFFFFE
        assert int(want[i]) == (key & 0xFFFFFFFF00000000) | (0xFFFFFFFF - to), i
    pos = hc.U32 - (keys & hc.U32)
    live = keys != 0
    assert (pos[live] == case.map_len - 1).any()  # the last entry of the map is asked for
    if case.count > 100:
        assert (~live).sum() == len(range(3, case.count, 7)) and (pos[live] == case.map_len).any()
        far = live & (pos >= case.map_len)
        assert far.sum() >= case.count // 14 and ((want[far] & hc.U32) == 1).all() and ((want[far] >> np.uint64(32)) == (keys[far] >> np.uint64(32))).all()


# ---- re-rank ---------------------------------------------------------------------------------------------------------------------------

def test_rerank_inputs_leave_no_doubt_about_the_order_and_the_oracle_answers_have_the_shapes():
    v, q = hc.rerank_corpus()
    s64 = np.sort(vo.scores_f64(v, q))[::-1]
    assert np.diff(-s64[:258]).min() > hc.RERANK_MIN_GAP  # the 256 best hits and the first that is not among them
    subset = hc.rerank_subset()
    sub64 = np.sort(vo.scores_f64(v[subset], q))[::-1]
    assert len(set(subset)) == len(subset) == 1200 and np.diff(-sub64[:258]).min() > hc.RERANK_MIN_GAP
    look = lambda e, k, t: vo.lookup(v, e, k, t)
    for case in hc.RERANK_CASES:
        rtm = hc.rerank_map(case.rows_map)
        n_messages = int(rtm.max()) + 1
        if case.form == "subset":
            if case.rows_map == "none":
                continue
            want = mo.memory_messages_from_hits(vo.lookup_in_subset(v, q, subset, case.max_matches, 0.0), rtm)
        else:
            accept = hc.rerank_accept(case.accept, n_messages)
            if case.accept.startswith("long"):
                assert len(accept) == hc.ACCEPT_LONG and (accept < n_messages).sum() == (150 if n_messages else 0)
                assert (np.flatnonzero(accept < n_messages) < 150).all() if case.accept == "long-head" else (np.flatnonzero(accept < n_messages) >= hc.ACCEPT_LONG - 150).all()
            want = mo.sqlite_lookup_by_embedding(look, q, rtm, case.max_matches, 0.0, accept)
        if case.rows_map == "one":
            assert len(want) == 1 and want[0][0] == 0  # every hit in one message
        elif case.rows_map == "none":
            assert want == []
        elif case.rows_map == "own" and case.accept == "none":
            assert len(want) == case.max_matches  # every hit in its own message
        elif case.rows_map == "own":
            assert 0 < len(want) < case.max_matches  # the accept collection drops hits
        elif case.accept == "none":
            assert len(want) == 1 if case.max_matches == 1 else 1 < len(want) <= case.max_matches
            if case.max_matches == 256:
                assert len(want) < 256  # several rows of a block among the hits collapse
