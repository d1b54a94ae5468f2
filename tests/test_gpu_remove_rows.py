"""GPU suite: removing rows.  tavb_compact_rows over the case table of tests/remove_rows_cases.py -- the device corpus afterwards is
np.delete of what was uploaded, bit for bit -- and `VectorBase.remove_rows` against a fresh index built from the np.delete'd matrix and
against the oracle."""

import numpy as np
import pytest

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests import remove_rows_cases as rc
from tests.synth import make_corpus, make_queries
from tests.test_gpu_parity import SCORE_TOL, assert_matches_expect, new_vb
from typeagent_py_amd import ScoredInt, _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = _native.Engine()
    yield eng
    eng.close()


def _dtype(name: str) -> int:
    return _native.TAVB_F16 if name == "f16" else _native.TAVB_F32


def _pairs(res):
    return [(r.item, r.score) for r in res]


@pytest.mark.parametrize("case", rc.cases(), ids=lambda c: c.id)
def test_compact_rows_equals_np_delete(engine, case):
    import torch

    eng = engine
    flags = rc.flags(case)
    eng.set_option("compact_pass_rows", case.pass_rows)
    try:
        eng.corpus, eng.rows, eng._owns_corpus = None, 0, False  # every case starts from a buffer of its own
        eng.upload_rows(np.ascontiguousarray(rc.matrix(case)), 0, _dtype(case.dtype))
        before = eng.corpus[: case.rows].cpu().numpy()  # what was uploaded, in the corpus' own dtype
        adopted = None
        if case.route == "out_of_place":
            adopted = eng.corpus[: case.rows].clone()
            eng.set_corpus_tensor(adopted)
            assert not eng._owns_corpus
        bits = eng.mask_bits_to_device(_native.pack_mask_bits(flags))
        torch.cuda.synchronize()
        kept = eng.compact_rows(bits)
        want = np.delete(before, np.flatnonzero(flags), axis=0)
        assert kept == len(want) == eng.rows
        got = eng.corpus[:kept].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        if adopted is not None:
            assert np.array_equal(adopted.cpu().numpy().view(np.uint8), before.view(np.uint8)), "an adopted tensor was written"
            if flags.any():
                assert eng.corpus is not adopted and eng._owns_corpus
            else:
                assert eng.corpus is adopted  # nothing to remove: nothing changes hands
    finally:
        eng.set_option("compact_pass_rows", 0)


def test_compact_rows_refuses_what_it_does_not_serve(engine):
    import torch

    eng = engine
    eng.corpus, eng.rows, eng._owns_corpus = None, 0, False
    eng.upload_rows(np.ascontiguousarray(rc.base_matrix(8)[:100]), 0, _native.TAVB_F32)
    bits = eng.mask_bits_to_device(_native.pack_mask_bits(np.arange(100) % 3 == 0))
    torch.cuda.synchronize()
    kept = _native.c_int64(0)
    h, lib = eng._h, eng.lib
    ptr = _native.c_void_p(bits.data_ptr())
    assert lib.tavb_compact_rows(h, ptr, 99, None, _native.byref(kept)) == -1 and b"covers 99 rows" in lib.tavb_last_error()
    assert lib.tavb_compact_rows(h, None, 100, None, _native.byref(kept)) == -1
    assert lib.tavb_compact_rows(h, ptr, 100, None, None) == -1
    assert lib.tavb_compact_rows(h, _native.c_void_p(bits.data_ptr() + 2), 100, None, _native.byref(kept)) == -1 and b"aligned" in lib.tavb_last_error()
    assert lib.tavb_compact_rows(h, ptr, 100, _native.c_void_p(eng.corpus.data_ptr() + 32), _native.byref(kept)) == -1 and b"overlaps" in lib.tavb_last_error()
    with pytest.raises(ValueError):
        eng.set_option("compact_pass_rows", -1)
    assert eng.rows == 100 and eng.get_option("compact_pass_rows") == 0
    assert eng.compact_rows(bits) == 66  # and the context still works


# ---- through the class ------------------------------------------------------------------------------------------------------------

def _class_setup(n, d, dtype, seed):
    v, q = make_corpus(n, d, seed)
    qs = np.concatenate([q[None], make_queries(69, d, seed + 1)])
    rng = np.random.default_rng(seed + 2)
    flags = rng.random(n) < 0.3
    flags[[0, n - 1]] = True
    flags[rc.CHUNK - 40 : rc.CHUNK + 40] = True  # a block over the chunk boundary
    row_to_msg = np.sort(rng.integers(0, n // 3, size=n)).astype(np.int64)
    row_to_msg[rng.choice(n, size=50, replace=False)] = -1
    ref = v.astype(np.float16).astype(np.float32) if dtype == "fp16" else v  # the values the kernels see
    return v, ref, qs, flags, row_to_msg


def _all_lookups(vb, qs, subset, mask_flags):
    out = {
        "single": _pairs(vb.fuzzy_lookup_embedding(qs[0], max_hits=32, min_score=0.0)),
        "subset": _pairs(vb.fuzzy_lookup_embedding_in_subset(qs[1], subset, max_hits=16, min_score=0.0)),
        "batch8": [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs[:8], max_hits=32, min_score=0.0)],
        "batch70": [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)],
        "masked": [_pairs(r) for r in vb.fuzzy_lookup_embeddings_masked(qs[:8], vb.row_mask(mask_flags), max_hits=16, min_score=0.0)],
        "messages": _pairs(vb.lookup_messages_by_embedding(qs[2], 25, 0.0)),
    }
    return out


def _check_against_oracle(got, ref, qs, subset, mask_flags, row_to_msg):
    """The project's usual rule (the helpers of tests/test_gpu_parity.py): ordinals identical, scores within 1e-5."""

    def same(res, want, scores, k):
        assert [i for i, _ in res] == [i for i, _ in want]
        assert_matches_expect([ScoredInt(i, s) for i, s in res], {"items": [i for i, _ in want], "scores": [s for _, s in want]}, scores, k, 0.0)

    same(got["single"], vo.lookup(ref, qs[0], 32, 0.0), vo.scores_full(ref, qs[0]), 32)
    same(got["subset"], vo.lookup_in_subset(ref, qs[1], subset, 16, 0.0), None, 16)
    for name, n in (("batch8", 8), ("batch70", 70)):
        for i in range(n):
            same(got[name][i], vo.lookup(ref, qs[i], 32, 0.0), vo.scores_full(ref, qs[i]), 32)
    allowed = np.flatnonzero(mask_flags).tolist()
    for i in range(8):
        same(got["masked"][i], vo.lookup_in_subset(ref, qs[i], allowed, 16, 0.0), None, 16)
    want = mo.sqlite_lookup_by_embedding(lambda e, k, t: vo.lookup(ref, e, k, t), qs[2], row_to_msg, 25, 0.0, None)
    assert [m for m, _ in got["messages"]] == [m for m, _ in want]
    np.testing.assert_allclose([s for _, s in got["messages"]], [s for _, s in want], atol=SCORE_TOL, rtol=0)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("n,d", [(rc.CHUNK + 1, 100), (2 * rc.CHUNK + 17, 384)])
def test_lookups_after_remove_rows_equal_a_fresh_index(n, d, dtype):
    v, ref, qs, flags, row_to_msg = _class_setup(n, d, dtype, 7100 + d)
    idx = np.flatnonzero(flags)
    vb = new_vb(v, dtype)
    vb.set_row_messages(row_to_msg)
    vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)  # the row-norm maxima and the fp16 shadow exist before the removal
    vb.lookup_messages_by_embedding(qs[2], 25, 0.0)
    eng = vb.engine
    tensor = eng.corpus
    assert vb.remove_rows(idx) == len(idx)
    assert len(vb) == n - len(idx) and eng.rows == len(vb) and eng.corpus is tensor  # compacted where it was: nothing uploaded again
    w = np.delete(v, idx, axis=0)
    fresh = new_vb(w, dtype)
    fresh.set_row_messages(np.delete(row_to_msg, idx))
    rng = np.random.default_rng(n + d)
    subset = rng.choice(len(w), size=500, replace=False).tolist()
    mask_flags = rng.random(len(w)) < 0.4
    got = _all_lookups(vb, qs, subset, mask_flags)
    assert vb.engine.corpus is tensor
    # a corpus this small sends the 70-query batch to the grouped streaming scan, which reads neither the shadow nor the maxima: the wide tile
    # is forced.  The removal dropped the maxima (row 0 went); this batch rebuilds them and filters on the rebuilt shadow
    grouped = eng.get_option("direct_group_max_nq")
    eng.set_option("direct_group_max_nq", 0)
    wide = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)]
    if dtype == "fp16" or d % 16 == 0:
        assert eng.get_option("last_tier") == 4 and eng.get_option("last_shadow") == int(dtype == "fp32" or d % 64 != 0) and eng.get_option("norm_rows") == len(w)
    else:  # fp32 rows of 100 floats: the wide tile does not serve the width, the streaming tiers take the batch and no cache is read
        assert eng.get_option("last_tier") == 2 and eng.get_option("norm_rows") == 0
    eng.set_option("direct_group_max_nq", grouped)
    assert wide == got["batch70"]  # the rescored wide tile carries the streaming kernels' scores: a stale shadow row would lose a true hit here
    want = _all_lookups(fresh, qs, subset, mask_flags)
    for name in want:
        assert got[name] == want[name], name  # bit for bit (the batches among them ran on the grouped streaming scan: no cache is read here)
    _check_against_oracle(got, np.delete(ref, idx, axis=0), qs, subset, mask_flags, np.delete(row_to_msg, idx))
    np.testing.assert_array_equal(np.asarray(vb.serialize()), w)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_remove_append_remove_with_lookups_between(dtype):
    n, d = rc.CHUNK + 1, 100
    v, ref, qs, flags, _ = _class_setup(n, d, dtype, 7300)
    extra, _ = make_corpus(300, d, 7301)
    vb = new_vb(v, dtype)
    model = v

    def check():
        fresh = new_vb(model, dtype)
        for q in qs[:3]:
            assert _pairs(vb.fuzzy_lookup_embedding(q, 20, 0.0)) == _pairs(fresh.fuzzy_lookup_embedding(q, 20, 0.0))
        assert [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, 20, 0.0)] == [_pairs(r) for r in fresh.fuzzy_lookup_embeddings(qs, 20, 0.0)]

    check()
    assert vb.remove_rows(flags) == int(flags.sum())
    model = np.delete(model, np.flatnonzero(flags), axis=0)
    check()
    vb.add_embeddings(None, extra)
    model = np.concatenate([model, extra])
    check()
    gone = [5, -1, 5, len(model) - 300]  # duplicates, a negative ordinal
    assert vb.remove_rows(gone) == 3
    model = np.delete(model, gone, axis=0)
    check()
    vb.remove_at(0)
    model = model[1:]
    check()
    assert len(vb) == len(model)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_device_only_corpus_is_compacted_without_a_host_copy(dtype):
    from tests.fakes import NullModel
    from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase

    n, d = 5000, 100
    v, ref, qs, _, _ = _class_setup(rc.CHUNK + 1, d, dtype, 7400)
    v, ref = v[:n], ref[:n]
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype, keep_host_copy=False)
    vb.add_embeddings(None, v)
    assert vb._device_only is not None
    flags = np.arange(n) % 7 == 3
    assert vb.remove_rows(flags) == int(flags.sum())
    assert vb._device_only is not None and vb._device_only is vb._engine.corpus and vb._host.shape[0] == 0
    w = np.delete(ref, np.flatnonzero(flags), axis=0)
    fresh = new_vb(np.delete(v, np.flatnonzero(flags), axis=0), dtype)
    assert _pairs(vb.fuzzy_lookup_embedding(qs[0], 20, 0.0)) == _pairs(fresh.fuzzy_lookup_embedding(qs[0], 20, 0.0))
    assert vb._device_only is not None
    np.testing.assert_array_equal(np.asarray(vb.serialize()), w)
    # an adopted tensor is never written: the index moves to a tensor of the engine's
    import torch

    t = torch.from_numpy(v).cuda()
    vb2 = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    vb2.adopt_device_corpus(t)
    assert vb2.remove_rows(flags) == int(flags.sum())
    assert np.array_equal(t.cpu().numpy(), v) and vb2._device_only is vb2._engine.corpus and vb2._device_only is not t
    np.testing.assert_array_equal(np.asarray(vb2.serialize()), np.delete(v, np.flatnonzero(flags), axis=0))


def test_stale_row_masks_raise_and_mask_removal_removes_its_rows():
    n, d = 3000, 64
    v, q = make_corpus(n, d, 7500)
    vb = new_vb(v)
    old = vb.row_mask(np.arange(n) % 2 == 0)
    a = vb.range_mask([[(100, 900)]])
    b = vb.range_mask([[(500, 1200), (2990, 4000)]])
    both = a & b
    gone = both.flat().copy()
    assert gone.tolist() == list(range(500, 900))
    assert vb.remove_rows(both) == 400
    np.testing.assert_array_equal(np.asarray(vb.serialize()), np.delete(v, gone, axis=0))
    for stale in (old, a, b, both):
        with pytest.raises(ValueError):
            vb.fuzzy_lookup_embedding_masked(q, stale, 5, 0.0)
    with pytest.raises(ValueError):
        vb.remove_rows(old)
    vb.add_embeddings(None, v[:400])  # back to the old length: the old handles still name other rows
    assert len(vb) == n
    with pytest.raises(ValueError, match="removed"):
        vb.fuzzy_lookup_embedding_masked(q, old, 5, 0.0)
    with pytest.raises(ValueError, match="removed"):
        old & vb.row_mask(np.ones(n, dtype=bool))
    assert len(vb.fuzzy_lookup_embedding_masked(q, vb.row_mask(np.arange(n) % 2 == 0), 5, 0.0)) == 5
    # a union mask built on the device, removed as it is
    u = vb.range_mask([[(0, 10)]]) | vb.range_mask([[(2995, 3000)]])
    keep = np.asarray(vb.serialize()).copy()
    assert vb.remove_rows(u) == 15
    np.testing.assert_array_equal(np.asarray(vb.serialize()), keep[10:2995])


def test_np_delete_errors_and_no_ops():
    n, d = 200, 16
    v, q = make_corpus(n, d, 7600)
    vb = new_vb(v)
    vb.fuzzy_lookup_embedding(q, 3, 0.0)
    mask = vb.row_mask(np.arange(n) < 5)
    for bad in ([n], [-n - 1], [0, 1, n + 7], np.array([3, 2 * n])):
        with pytest.raises(IndexError, match="out of bounds"):
            vb.remove_rows(bad)
    with pytest.raises(IndexError):
        vb.remove_rows([1.5])
    with pytest.raises(ValueError):
        vb.remove_rows(np.zeros(n - 1, dtype=bool))
    with pytest.raises(IndexError, match=f"Index {n} out of bounds for embedding index of size {n}"):
        vb.remove_at(n)
    with pytest.raises(IndexError):
        vb.remove_at(-1)
    assert vb.remove_rows([]) == 0 and vb.remove_rows(np.zeros(n, dtype=bool)) == 0 and vb.remove_rows(np.zeros(0, dtype=np.int64)) == 0
    assert len(vb) == n and len(vb.fuzzy_lookup_embedding_masked(q, mask, 3, 0.0)) == 3  # a no-op leaves the handles alone
    assert vb.remove_rows(np.ones(n, dtype=bool)) == n and len(vb) == 0
    assert vb.fuzzy_lookup_embedding(q, 3, 0.0) == []
    assert vb.remove_rows([]) == 0
    vb.add_embeddings(None, v[:10])
    assert [r.item for r in vb.fuzzy_lookup_embedding(v[4], 1, 0.0)] == [4]
