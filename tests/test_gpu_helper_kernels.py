"""GPU suite: the helper kernels of csrc/tavb_misc.hip on every branch (the table is tests/helper_kernel_cases.py; its CPU twin
tests/test_helper_kernel_cases_host.py asserts that every branch has a case and checks the numpy references).

  * `merge_kernel` through `Engine.merge_device` (the list-major layout of the N > 1 exchange): 1 .. 100 lists of k = 1 .. 256 keys -- both
    register forms, odd counts, more lists than waves, the four-lists-per-round loop, ragged, empty and one-list fills, equal score bits,
    ordinals next to 2^32 - 2, a list of failure keys -- against the descending uint64 sort of the union and the host twin `merge_keys`.
    One GPU folding 8 lists is what stands in for the 8-GPU answer.
  * `normalize_rows_kernel<6 / 16 / 0>`, in place and out of place: every width class, the unaligned fall-back, the grid-stride loop; NaN, inf
    and overflowing rows exactly as numpy; finite rows inside the worst-case float64 bound of the kernel's own summation AND an exact IEEE
    float32 quotient (no reciprocal-multiply).
  * `f32_to_f16_kernel` bit for bit against numpy's cast: vector body, scalar tail, unaligned branch, grid-stride loop, overflow, half
    subnormals, ties; and the load path that rides it (`upload_rows`): a three-chunk fp16 corpus of odd width and appends at odd rows,
    read back bit for bit and tied to a lookup.
  * `remap_positions_kernel`: zero keys, positions behind the map, more keys than the grid.
  * `message_rerank_kernel` / `accept_bitmap_kernel` against oracle/messages_oracle.py: k = 256, every hit in one message, every hit in its
    own, no hit with a message, an accept collection longer than the bitmap kernel's grid.

Every pointer is valid and every length inside its buffer; the unaligned views are 4-byte aligned views into larger buffers, and the
elements around them are checked to be untouched.  Every test runs under a watchdog of its own and nothing is retried."""

from __future__ import annotations

import faulthandler

import numpy as np
import pytest

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests import helper_kernel_cases as hc
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native
from typeagent_py_amd.adapters import lookup_messages_by_embedding, lookup_messages_in_subset

pytestmark = pytest.mark.gpu

TEST_LIMIT_S = 120
SCORE_TOL = 1e-5
GUARD = 12345.0  # in the floats around an unaligned view


@pytest.fixture(autouse=True)
def watchdog():
    faulthandler.dump_traceback_later(TEST_LIMIT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def eng():
    e = _native.Engine(0)
    yield e
    e.close()


def _torch():
    import torch

    return torch


def _device_view(x: np.ndarray, offset: int):
    """`x` on the device, its first element `offset` floats behind a 16-byte boundary: (the buffer, the view)"""
    torch = _torch()
    flat = torch.full((x.size + 8,), GUARD, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[offset : offset + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 * offset
    return flat, view


def _assert_guards(flat, offset: int, size: int, what: str):
    host = flat.cpu().numpy()
    assert (host[:offset] == GUARD).all() and (host[offset + size:] == GUARD).all(), f"{what}: written outside the view"


# ---- 1. merge --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.MERGE_CASES, ids=[c.name for c in hc.MERGE_CASES])
def test_merge_device(eng, case):
    torch = _torch()
    lists = hc.merge_lists(case)
    want = hc.merged_by_sort(lists)
    np.testing.assert_array_equal(_native.merge_keys(lists), want, err_msg=f"{case.name}: the host twin")
    dl = torch.from_numpy(lists.view(np.int64)).cuda()
    out = torch.full((case.nq + 1, case.k), -1, dtype=torch.int64, device="cuda")  # a row behind the last query: must stay as it is
    torch.cuda.synchronize()
    eng.merge_device(dl, out_keys=out)
    eng.synchronize()
    got = out.cpu().numpy().view(np.uint64)
    assert (got[case.nq] == hc.FAILED).all(), f"{case.name}: keys written behind the last query"
    diff = got[: case.nq] != want
    assert not diff.any(), (f"{case.name} ({sorted(hc.merge_branches(case.n_lists, case.k))}): {int(diff.sum())} of {want.size} keys differ from the sort of the "
                            f"union; first at (query, slot) {np.argwhere(diff)[:6].tolist()}")
    if case.fill == "failed":  # the query of the failed rank leads with the failure key and decoding raises; the other queries are whole
        assert got[1, 0] == hc.FAILED and (got[[0, 2]] != hc.FAILED).all()
        with pytest.raises(_native.TavbError, match="a rank of the collective lookup failed"):
            _native.decode_keys(got[: case.nq])
        ords, _, cnts = _native.decode_keys(got[[0, 2]])
        assert (cnts == case.k).all() and (ords >= 0).all()


# ---- 2. normalise ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.NORM_CASES, ids=[c.name for c in hc.NORM_CASES])
def test_normalize_rows(eng, case):
    x = hc.norm_input(case)
    with np.errstate(over="ignore", invalid="ignore"):
        oracle = vo.l2_normalize_rows(x)
    flat, view = _device_view(x, case.offset)
    y = eng.normalize_rows(view).cpu().numpy()
    np.testing.assert_array_equal(view.cpu().numpy().view(np.uint32), x.view(np.uint32), err_msg=f"{case.name}: the input of the out-of-place call changed")
    fig = hc.norm_check(case, x, y, oracle, "out of place")
    print(f"{case.name} {sorted(hc.norm_branch(case))}: worst element {fig['worst_units']:.2f} of {fig['bound_units']} units of 2^-24, "
          f"norm {fig['norm_steps']} float32 steps from the float64 norm")
    eng.normalize_rows_(view)
    y2 = view.cpu().numpy()
    _assert_guards(flat, case.offset, x.size, case.name)
    hc.norm_check(case, x, y2, oracle, "in place")
    np.testing.assert_array_equal(y2.view(np.uint32), y.view(np.uint32), err_msg=f"{case.name}: in place and out of place differ")


# ---- 3. convert and the load path ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.CONV_CASES, ids=[c.name for c in hc.CONV_CASES])
def test_to_f16(eng, case):
    x = hc.conv_input(case)
    flat, view = _device_view(x, case.offset)
    y = eng.to_f16(view).cpu().numpy()
    hc.conv_check(x, y, f"{case.name} {sorted(hc.conv_branches(case))}")
    _assert_guards(flat, case.offset, x.size, case.name)


@pytest.mark.parametrize("case", hc.UPLOAD_CASES, ids=[c.name for c in hc.UPLOAD_CASES])
def test_upload_rows(case):
    torch = _torch()
    v, q = hc.upload_input(case)
    e = _native.Engine(0)
    start = 0
    for n in case.parts:
        e.upload_rows(v[start : start + n], start, _native.TAVB_F16 if case.dtype == "fp16" else _native.TAVB_F32)
        start += n
    assert e.rows == case.rows and e.dim == case.dim and e.corpus.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    back = e.corpus[: case.rows].cpu().numpy()
    chunks = hc.upload_chunks(case)
    if case.dtype == "fp32":
        assert back.dtype == np.float32
        np.testing.assert_array_equal(back.view(np.uint32), v.view(np.uint32), err_msg=case.name)
        e.close()
        return
    assert back.dtype == np.float16 and any(off % 16 for _, _, off in chunks)
    want = v.astype(np.float16)
    for first, n, off in chunks:  # chunk by chunk, so that a failure names the chunk and its alignment
        diff = back[first : first + n].view(np.uint16) != want[first : first + n].view(np.uint16)
        assert not diff.any(), (f"{case.name}: rows {first} .. {first + n - 1} (destination {off} bytes behind a 16-byte boundary): {int(diff.sum())} elements differ; "
                                f"first at {(np.argwhere(diff)[:4] + [first, 0]).tolist()}")
    # one lookup ties the rows on the device to the answer
    rounded = want.astype(np.float32)
    ords, scs = e.search(q, 10, _native.f32_threshold(0.0))
    assert len(ords) == 10
    vo.check_topk_parity(vo.scores_full(rounded, q), ords, scs, 10, 0.0, referee=vo.f64_referee(rounded, q))
    e.close()


# ---- 4. remap --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", hc.REMAP_CASES, ids=[c.name for c in hc.REMAP_CASES])
def test_remap_key_positions(eng, case):
    torch = _torch()
    keys, m = hc.remap_input(case)
    want = hc.remap_reference(keys, m)
    dk = torch.full((case.count + 2,), -1, dtype=torch.int64, device="cuda")  # a guard key on either side
    dk[1:-1].copy_(torch.from_numpy(keys.view(np.int64)))
    dm = torch.from_numpy(m).cuda()
    torch.cuda.synchronize()
    eng.remap_key_positions(dk[1:-1], dm)
    eng.synchronize()
    got = dk.cpu().numpy().view(np.uint64)
    assert got[0] == hc.FAILED and got[-1] == hc.FAILED, f"{case.name}: written outside the keys"
    diff = got[1:-1] != want
    assert not diff.any(), f"{case.name}: {int(diff.sum())} of {case.count} keys differ; first at {np.flatnonzero(diff)[:6].tolist()}"
    assert (got[1:-1][keys == 0] == 0).all()


# ---- 5. re-rank ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rerank_index():
    v, q = hc.rerank_corpus()
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb.add_embeddings(None, np.ascontiguousarray(v, dtype=np.float32))
    return v, q, vb


@pytest.mark.parametrize("case", hc.RERANK_CASES, ids=[c.name for c in hc.RERANK_CASES])
def test_message_rerank(rerank_index, case):
    v, q, vb = rerank_index
    rtm = hc.rerank_map(case.rows_map)
    n_messages = int(rtm.max()) + 1
    if case.form == "subset":
        subset = hc.rerank_subset()
        got = lookup_messages_in_subset(vb, q, subset, rtm, max_matches=case.max_matches, threshold_score=0.0)
        # (the memory provider has no row without a message: with the all -1 map the kernel's answer is the empty list)
        want = [] if case.rows_map == "none" else mo.memory_messages_from_hits(vo.lookup_in_subset(v, q, subset, case.max_matches, 0.0), rtm)
    else:
        accept = hc.rerank_accept(case.accept, n_messages)
        got = lookup_messages_by_embedding(vb, q, rtm, max_matches=case.max_matches, threshold_score=0.0, accept=accept)
        want = mo.sqlite_lookup_by_embedding(lambda e, k, t: vo.lookup(v, e, k, t), q, rtm, case.max_matches, 0.0, accept)
    assert [h.item for h in got] == [m for m, _ in want], case.name
    np.testing.assert_allclose([h.score for h in got], [s for _, s in want], atol=SCORE_TOL, rtol=0, err_msg=case.name)
    if case.rows_map == "one":
        assert len(got) == 1
    elif case.rows_map == "none":
        assert got == []
    elif case.rows_map == "own" and case.accept == "none":
        assert len(got) == case.max_matches
