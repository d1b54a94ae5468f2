"""GPU suite: inserting and overwriting rows.  tavb_expand_rows + tavb_scatter_rows over the case table of tests/insert_rows_cases.py --
the device corpus afterwards is np.insert of what was uploaded, bit for bit -- rows whose values fp16 rounds, against a fresh upload;
`VectorBase.insert_rows` / `set_rows` on a device-only and on a mirrored corpus against a fresh index built from numpy's result; the
caches `set_rows` keeps; and the arguments both calls refuse."""

import numpy as np
import pytest

from tests import insert_rows_cases as ic
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from tests.test_gpu_parity import new_vb
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    eng = _native.Engine()
    yield eng
    eng.close()


def _dtype(name: str) -> int:
    return _native.TAVB_F16 if name in ("f16", "fp16") else _native.TAVB_F32


def _pairs(res):
    return [(r.item, r.score) for r in res]


def _fresh_engine_corpus(eng, rows: np.ndarray, dtype: int, capacity: int = 0):
    eng.corpus, eng.rows, eng._owns_corpus = None, 0, False  # every case starts from a buffer of its own
    eng.upload_rows(np.ascontiguousarray(rows, dtype=np.float32), 0, dtype, capacity_hint=capacity)


@pytest.mark.parametrize("case", ic.cases(), ids=lambda c: c.id)
def test_expand_and_scatter_equal_np_insert(engine, case):
    import torch

    eng = engine
    at, holes = ic.at(case), ic.holes(case)
    old, new = ic.old_matrix(case), ic.new_matrix(case)
    n, m = len(old), len(new)
    pos = ic.positions_of(at, n)
    eng.set_option("compact_pass_rows", case.pass_rows)
    try:
        _fresh_engine_corpus(eng, old, _dtype(case.dtype), capacity=case.rows if case.route == "in_place" else 0)
        before = eng.corpus[:n].cpu().numpy()  # what was uploaded, in the corpus' own dtype
        adopted = None
        if case.route == "adopted":
            adopted = eng.corpus[:n].clone()
            eng.set_corpus_tensor(adopted)
            assert not eng._owns_corpus
        elif case.route == "no_capacity":
            eng.set_corpus_tensor(eng.corpus[:n].clone(), _owned=True)  # a buffer of the engine's with not one spare row
        tensor = eng.corpus
        bits = eng.mask_bits_to_device(_native.pack_mask_bits(holes))
        torch.cuda.synchronize()
        assert eng.expand_rows(bits, case.rows) == n and eng.rows == case.rows
        eng.scatter_rows(new, pos.astype(np.int32))
        want = np.insert(before, at, new.astype(before.dtype), axis=0) if m else before
        assert len(want) == case.rows == eng.rows
        got = eng.corpus[: case.rows].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        if m == 0 or case.route == "in_place":
            assert eng.corpus is tensor  # nothing to insert: nothing changes hands; room to spare: expanded where it was
        else:
            assert eng.corpus is not tensor and eng._owns_corpus and eng.corpus.shape[0] >= max(case.rows, 2 * tensor.shape[0], 16)
        if adopted is not None:
            assert np.array_equal(adopted.cpu().numpy().view(np.uint8), before.view(np.uint8)), "an adopted tensor was written"
    finally:
        eng.set_option("compact_pass_rows", 0)


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_rows_that_fp16_rounds_equal_a_fresh_upload(engine, dtype):
    eng = engine
    n, m, d = 300, 77, 100
    v, _ = make_corpus(n + m, d, 9900)  # unit rows of random floats: none exact in fp16
    assert not np.array_equal(v.astype(np.float16).astype(np.float32), v)
    rng = np.random.default_rng(9901)
    at = rng.integers(-n, n + 1, size=m)
    old, new = v[:n], v[n:]
    want_host = np.insert(old, at, new, axis=0)
    _fresh_engine_corpus(eng, want_host, _dtype(dtype))
    want = eng.corpus[: n + m].cpu().numpy()
    _fresh_engine_corpus(eng, old, _dtype(dtype), capacity=n + m)
    pos = ic.positions_of(at, n)
    holes = np.zeros(n + m, dtype=bool)
    holes[pos] = True
    assert eng.expand_rows(eng.mask_bits_to_device(_native.pack_mask_bits(holes)), n + m) == n
    eng.scatter_rows(new, pos.astype(np.int32))
    got = eng.corpus[: n + m].cpu().numpy()
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))
    # overwritten rows as well
    which = rng.choice(n + m, size=50, replace=False)
    want_host[which] = -v[:50]
    eng.scatter_rows(-v[:50], which.astype(np.int32))
    got = eng.corpus[: n + m].cpu().numpy()
    _fresh_engine_corpus(eng, want_host, _dtype(dtype))
    assert np.array_equal(got.view(np.uint8), eng.corpus[: n + m].cpu().numpy().view(np.uint8))


def test_bad_arguments_are_errors_and_move_nothing(engine):
    import torch

    eng = engine
    old = ic.base_matrix(8)[:100]
    _fresh_engine_corpus(eng, old, _native.TAVB_F32, capacity=200)
    holes = np.arange(130) % 4 == 0  # 33 holes: 97 clear bits, not 100
    bits = eng.mask_bits_to_device(_native.pack_mask_bits(holes))
    torch.cuda.synchronize()
    out = _native.c_int64(0)
    h, lib = eng._h, eng.lib
    ptr = _native.c_void_p(bits.data_ptr())
    assert lib.tavb_expand_rows(h, ptr, 130, None, _native.byref(out)) == -1 and b"the corpus has 100" in lib.tavb_last_error() and out.value == 97
    with pytest.raises(Exception):
        eng.expand_rows(bits, 130)
    assert lib.tavb_expand_rows(h, ptr, 99, None, _native.byref(out)) == -1  # fewer rows than there are
    assert lib.tavb_expand_rows(h, None, 130, None, _native.byref(out)) == -1
    assert lib.tavb_expand_rows(h, ptr, 130, None, None) == -1
    assert lib.tavb_expand_rows(h, _native.c_void_p(bits.data_ptr() + 2), 130, None, _native.byref(out)) == -1 and b"aligned" in lib.tavb_last_error()
    good = np.zeros(133, dtype=bool)
    good[:132:4] = True  # 33 holes, 100 clear bits
    assert (~good).sum() == 100
    gbits = eng.mask_bits_to_device(_native.pack_mask_bits(good))
    torch.cuda.synchronize()
    overlapping = _native.c_void_p(eng.corpus.data_ptr() + 32)
    assert lib.tavb_expand_rows(h, _native.c_void_p(gbits.data_ptr()), 133, overlapping, _native.byref(out)) == -1 and b"overlaps" in lib.tavb_last_error()
    rows = np.ones((3, 8), dtype=np.float32)
    for bad in ([0, 100, 1], [-1, 2, 3]):
        with pytest.raises(Exception, match="outside"):
            eng.scatter_rows(rows, np.array(bad, dtype=np.int32))
    with pytest.raises(ValueError):
        eng.scatter_rows(rows, np.array([1, 2], dtype=np.int32))
    with pytest.raises(ValueError):
        eng.scatter_rows(np.ones((3, 9), dtype=np.float32), np.array([1, 2, 3], dtype=np.int32))
    assert eng.rows == 100 and np.array_equal(eng.corpus[:100].cpu().numpy(), old)  # nothing moved, nothing was written
    assert eng.expand_rows(gbits, 133) == 100 and eng.rows == 133  # and the context still works
    assert np.array_equal(eng.corpus[:133].cpu().numpy()[~good], old)


# ---- through the class ------------------------------------------------------------------------------------------------------------

N, D = 5000, 128


def _all_lookups(vb, qs, mask_flags):
    return {
        "single": _pairs(vb.fuzzy_lookup_embedding(qs[0], max_hits=32, min_score=0.0)),
        "batch8": [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs[:8], max_hits=32, min_score=0.0)],
        "batch128": [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)],
        "masked": [_pairs(r) for r in vb.fuzzy_lookup_embeddings_masked(qs[:8], vb.row_mask(mask_flags), max_hits=16, min_score=0.0)],
        "messages": _pairs(vb.lookup_messages_by_embedding(qs[2], 25, 0.0)),
    }


def _index(v, dtype, storage):
    if storage == "mirrored":
        return new_vb(v, dtype)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype, keep_host_copy=False)
    vb.add_embeddings(None, v)
    assert vb._device_only is not None
    return vb


@pytest.mark.parametrize("storage", ["device_only", "mirrored"])
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_lookups_after_insert_rows_and_set_rows_equal_a_fresh_index(dtype, storage):
    v, q = make_corpus(N, D, 9950)
    extra, _ = make_corpus(700, D, 9951)
    qs = np.concatenate([q[None], make_queries(127, D, 9952)])
    rng = np.random.default_rng(9953)
    row_to_msg = np.sort(rng.integers(0, N // 3, size=N)).astype(np.int64)
    vb = _index(v, dtype, storage)
    vb.set_row_messages(row_to_msg)
    vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)  # the row-norm maxima (and the shadow) exist before the edits
    vb.lookup_messages_by_embedding(qs[2], 25, 0.0)

    def check(model, msgs):
        if storage == "device_only":
            assert vb._device_only is not None and vb._device_only is vb._engine.corpus and vb._host.shape[0] == 0  # never copied to the host
        assert len(vb) == len(model) == vb._engine.rows
        fresh = new_vb(model, dtype)
        fresh.set_row_messages(msgs)
        mask_flags = np.random.default_rng(len(model)).random(len(model)) < 0.4
        got, want = _all_lookups(vb, qs, mask_flags), _all_lookups(fresh, qs, mask_flags)
        for name in want:
            assert got[name] == want[name], name  # bit for bit
        # a corpus this small sends the 128-query batch to the grouped streaming scan, which reads neither the shadow nor the maxima: the wide
        # tile is forced, and a stale shadow or stale norm maxima show HERE
        eng = vb.engine
        grouped = eng.get_option("direct_group_max_nq")
        eng.set_option("direct_group_max_nq", 0)
        wide = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=32, min_score=0.0)]
        assert eng.get_option("last_tier") == 4 and eng.get_option("last_shadow") == int(dtype == "fp32") and eng.get_option("norm_rows") == len(model)
        eng.set_option("direct_group_max_nq", grouped)
        assert wide == want["batch128"]

    at = np.concatenate([[0, 0, N, -1], rng.integers(-N, N + 1, size=496)])
    new_msgs = rng.integers(0, N // 3, size=500)
    assert vb.insert_rows(at, extra[:500], row_messages=new_msgs) == 500
    model, msgs = np.insert(v, at, extra[:500], axis=0), np.insert(row_to_msg, at, new_msgs)
    check(model, msgs)
    which = np.concatenate([[0, -1, 7, 7], rng.choice(len(model), size=196, replace=False)])  # a duplicate: the last one wins
    assert vb.set_rows(which, extra[500:]) == len(set((which % len(model)).tolist()))
    model[which] = extra[500:]
    check(model, msgs)
    assert vb.insert_rows(len(model) // 2, extra[:3]) == 3  # and once more after the overwrite
    check(np.insert(model, len(model) // 2, extra[:3], axis=0), np.insert(msgs, len(model) // 2, [-1, -1, -1]))
    if storage == "mirrored":
        np.testing.assert_array_equal(np.asarray(vb.serialize()), np.insert(model, len(model) // 2, extra[:3], axis=0))


@pytest.mark.parametrize("dtype,d", [("fp32", 128), ("fp16", 100)])
def test_set_rows_keeps_the_shadow_and_folds_the_norms(dtype, d):
    """fp32: the fp16 shadow; fp16 rows of a width that is no multiple of 64: the zero-padded copy.  Both are filled on the first large
    batch together with the row-norm maxima ("norm_rows" rows of them), and `set_rows` must leave all three usable."""
    v, q = make_corpus(N, d, 9960)
    extra, _ = make_corpus(40, d, 9961)
    qs = np.concatenate([q[None], make_queries(127, d, 9962)])
    vb = new_vb(v, dtype)
    eng = vb.engine
    eng.set_option("small_direct_bytes", 0)  # (a corpus this small would otherwise take the grouped streaming scan)
    first = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=16, min_score=0.0)]
    assert eng.get_option("last_shadow") == 1 and eng.get_option("norm_rows") == N
    model = v.copy()
    which = np.arange(3, N, 113)[:40]
    assert len(which) == 40
    rows = extra.copy()
    rows[5] *= 4.0  # a norm four times every old one: the cached maxima must grow, or the filter's bound is wrong for this row
    qs[7] = rows[5] / 4.0
    assert vb.set_rows(which, rows) == 40
    model[which] = rows
    assert eng.get_option("norm_rows") == N, "set_rows threw the row-norm maxima and the shadow away"
    got = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, max_hits=16, min_score=0.0)]
    assert eng.get_option("last_shadow") == 1 and eng.get_option("norm_rows") == N
    fresh = new_vb(model, dtype)
    fresh.engine.set_option("small_direct_bytes", 0)
    want = [_pairs(r) for r in fresh.fuzzy_lookup_embeddings(qs, max_hits=16, min_score=0.0)]
    assert fresh.engine.get_option("last_shadow") == 1
    assert got == want and got != first
    assert got[7][0][0] == int(which[5])  # the scaled row leads its own query, as it does on the streaming kernel
    assert vb.fuzzy_lookup_embedding(qs[7], max_hits=1, min_score=0.0)[0].item == int(which[5])
