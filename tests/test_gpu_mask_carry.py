"""GPU suite: `RowMask` handles carried through row edits on the device (tavb_mask_remap).  Over the case table of
tests/mask_carry_cases.py every carried handle equals a fresh `row_mask` of numpy's delete / insert / concatenate -- count, span, packed
words, row list; the engine call ignores garbage behind the inputs' rows and refuses flags that do not describe the edit; carried and
fresh handles answer every masked route bit for bit; an edit sequence carries its handles across every step; a device-only corpus stays
on the device."""

import numpy as np
import pytest

from tests import mask_carry_cases as mc
from tests.fakes import NullModel
from tests.synth import make_queries
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu


def new_vb(v, dtype="fp16", **kw) -> VectorBase:
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype, **kw)
    vb.add_embeddings(None, np.ascontiguousarray(v, dtype=np.float32))
    return vb


def assert_same_handle(got, want, what=""):
    """A carried handle against a fresh one of the same index: count, span, the packed words below `rows` (tail bits zero), the row list."""
    assert got.rows == want.rows and got.epoch == want.epoch and got.count == want.count and got.span == want.span, (what, got.rows, want.rows, got.count, want.count, got.span, want.span)
    assert got._plans == {} and got._flat is None and got.dev_bits is not None and got.dev_rows is not None, what
    n_words = (got.rows + 31) // 32
    a, b = got.dev_bits.cpu().numpy().view(np.uint32), want.dev_bits.cpu().numpy().view(np.uint32)
    assert len(a) == n_words and np.array_equal(a, b[:n_words]), what
    if got.rows % 32:
        assert int(a[-1]) >> (got.rows % 32) == 0, what
    assert np.array_equal(got.dev_rows.cpu().numpy(), want.dev_rows.cpu().numpy()) and got.dev_rows.shape[0] == got.count, what


def apply_case(vb: VectorBase, c: mc.Case, handles):
    if c.mode == "remove":
        f = mc.flags(c)
        assert vb.remove_rows(f, carry=handles) == int(f.sum())
    elif c.mode == "insert":
        at, m = mc.insertion(c.kind, c.rows)
        assert vb.insert_rows(at, mc.new_vectors(c), carry=handles, carry_new=c.fill) == m
    else:
        vb.add_embeddings(None, np.array(mc.new_vectors(c)))
        vb.extend_masks(*handles, new=c.fill)
    assert len(vb) == mc.new_rows(c)


@pytest.mark.parametrize("case", mc.cases(), ids=lambda c: c.id)
def test_a_carried_handle_equals_a_fresh_one(case):
    vb = new_vb(mc.old_matrix(case), case.dtype)
    handles = [vb.row_mask(b) for b in mc.masks(case)]
    assert all(h.dev_bits is not None for h in handles)
    apply_case(vb, case, handles)
    for i, (h, want) in enumerate(zip(handles, mc.expected(case))):
        if len(want) == 0:
            assert h.rows == 0 and h.count == 0 and h.epoch == vb._removal_epoch
            continue
        assert_same_handle(h, vb.row_mask(want), f"{case.id} mask {i}")


def test_a_removal_by_a_carried_handle_leaves_it_empty():
    n = mc.CHUNK + 1
    vb = new_vb(mc.base_matrix()[:n])
    f = mc.removal("random_50", n)
    which, other = vb.row_mask(f), vb.row_mask(~f)
    assert vb.remove_rows(which, carry=[other, which]) == int(f.sum())
    assert which.count == 0 and which.span is None and which.rows == len(vb) and not which.dev_bits.cpu().numpy().any()
    assert_same_handle(other, vb.row_mask(np.ones(len(vb), dtype=bool)))


# ---- the engine call ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def engine():
    eng = _native.Engine()
    yield eng
    eng.close()


def _quads(eng, mode, flags, old, new, masks, fill, garbage, counts=None):
    """`mask_remap` over numpy bool masks -> [(rows, count, words, span)] as numpy; garbage: the inputs are two words longer than needed
    and every bit at or beyond `old` is set."""
    import torch

    ins = []
    for b in masks:
        words = _native.pack_mask_bits(b)
        if garbage:
            words = np.concatenate([words, np.full(2, 0xFFFFFFFF, dtype=np.uint32)])
            if old % 32:
                words[old // 32] |= np.uint32((0xFFFFFFFF << (old % 32)) & 0xFFFFFFFF)
        ins.append(eng.mask_bits_to_device(words))
    dev_flags = None if flags is None else eng.mask_bits_to_device(_native.pack_mask_bits(flags))
    torch.cuda.synchronize()
    out = eng.mask_remap(mode, dev_flags, old, new, ins, fill, counts=counts)
    return [(r.cpu().numpy(), n, w.cpu().numpy().view(np.uint32), span) for r, n, w, span in out]


@pytest.mark.parametrize("mode", ["remove", "insert", "append"])
def test_the_engine_call_ignores_bits_behind_the_inputs_rows(engine, mode):
    c = next(c for c in mc.cases() if c.mode == mode and c.rows == 2 * mc.CHUNK + 17 and c.n_masks == 8)
    code = {"remove": _native.REMAP_REMOVE, "insert": _native.REMAP_INSERT, "append": _native.REMAP_APPEND}[mode]
    flags = None if mode == "append" else mc.flags(c)
    clean = _quads(engine, code, flags, c.rows, mc.new_rows(c), mc.masks(c), c.fill, garbage=False, counts=[int(b.sum()) for b in mc.masks(c)])
    dirty = _quads(engine, code, flags, c.rows, mc.new_rows(c), mc.masks(c), c.fill, garbage=True)
    for (r0, n0, w0, s0), (r1, n1, w1, s1), want in zip(clean, dirty, mc.expected(c)):
        assert n0 == n1 == int(want.sum()) and s0 == s1 and np.array_equal(r0, r1) and np.array_equal(w0, w1)
        assert np.array_equal(w0, _native.pack_mask_bits(want)) and np.array_equal(r0, np.flatnonzero(want))
        assert s0 == ((int(np.flatnonzero(want)[0]), int(np.flatnonzero(want)[-1])) if want.any() else None)


def test_flags_that_do_not_describe_the_edit_are_refused(engine):
    import torch

    eng = engine
    n = mc.CHUNK + 1
    f = mc.removal("random_1", n)
    kept = n - int(f.sum())
    b = np.arange(n) % 3 == 0
    for mode, old, new in ((_native.REMAP_REMOVE, n, kept - 1), (_native.REMAP_REMOVE, n, kept + 1), (_native.REMAP_INSERT, kept - 1, n), (_native.REMAP_INSERT, kept + 1, n)):
        dev_flags = eng.mask_bits_to_device(_native.pack_mask_bits(f))
        dev_in = eng.mask_bits_to_device(_native.pack_mask_bits(b[:old]))
        torch.cuda.synchronize()
        with pytest.raises(ValueError, match="clear bits"):
            eng.mask_remap(mode, dev_flags, old, new, [dev_in], False)
    with pytest.raises(ValueError):
        eng.mask_remap(_native.REMAP_REMOVE, None, 10, 11, [eng.mask_bits_to_device(_native.pack_mask_bits(b[:10]))], False)
    with pytest.raises(ValueError, match="1 .. 8"):
        eng.mask_remap(_native.REMAP_APPEND, None, 10, 11, [], False)
    # an output is nobody's input: the C call refuses an output that overlaps the flags
    dev_flags = eng.mask_bits_to_device(_native.pack_mask_bits(f))
    dev_in = eng.mask_bits_to_device(_native.pack_mask_bits(b))
    torch.cuda.synchronize()
    infos = (_native.MaskInfo * 1)()
    ins = (_native.c_void_p * 1)(dev_in.data_ptr())
    outs = (_native.c_void_p * 1)(dev_flags.data_ptr())
    rc = eng.lib.tavb_mask_remap(eng._h, _native.REMAP_REMOVE, _native.c_void_p(dev_flags.data_ptr()), n, kept, ins, outs, 1, 0, None, None, infos)
    assert rc == -1 and b"overlaps the flags" in eng.lib.tavb_last_error()
    assert np.array_equal(dev_flags.cpu().numpy().view(np.uint32), _native.pack_mask_bits(f))
    # the same call with an output of its own: the right answer
    (rows, count, words, span), = _quads(eng, _native.REMAP_REMOVE, f, n, kept, [b], False, garbage=False)
    assert count == int(b[~f].sum()) and np.array_equal(words, _native.pack_mask_bits(b[~f]))


# ---- carried and fresh handles answer alike -------------------------------------------------------------------------------------------------------

def _hits(lists):
    return [[(r.item, r.score) for r in one] for one in lists]


@pytest.mark.parametrize("dtype", mc.DTYPES)
@pytest.mark.parametrize("rows", mc.AROUND_CHUNK)
def test_carried_and_fresh_handles_answer_bit_for_bit(rows, dtype):
    v = mc.base_matrix()[:rows]
    vb = new_vb(v, dtype)
    rng = np.random.default_rng(rows)
    a0, b0 = rng.random(rows) < 0.5, np.arange(rows) % 3 != 0
    gone = mc.removal("random_1", rows)
    msgs = np.arange(rows) // 3
    vb.set_row_messages(msgs)
    a, b = vb.row_mask(a0), vb.row_mask(b0)
    assert vb.remove_rows(gone, carry=[a, b]) == int(gone.sum())
    a1, b1 = a0[~gone], b0[~gone]
    fa, fb = vb.row_mask(a1), vb.row_mask(b1)
    qs = make_queries(130, mc.DIM, rows)
    eng = vb.engine
    assert _hits([vb.fuzzy_lookup_embedding_masked(qs[0], a, 10, 0.0)]) == _hits([vb.fuzzy_lookup_embedding_masked(qs[0], fa, 10, 0.0)])
    routes = [(0, 0, 1, 9), (2, 0, 2, 64)] + ([(0, 2, 3, 130)] if dtype == "fp16" else [])
    try:
        for tile, wide, route, nq in routes:
            eng.set_option("mask_tile", tile)
            eng.set_option("mask_wide", wide)
            got = vb.fuzzy_lookup_embeddings_masked(qs[:nq], a, 10, 0.0)
            assert eng.get_option("masked_route") == route, (tile, wide)
            want = vb.fuzzy_lookup_embeddings_masked(qs[:nq], fa, 10, 0.0)
            assert eng.get_option("masked_route") == route and _hits(got) == _hits(want), (tile, wide)
    finally:
        eng.set_option("mask_tile", 1)
        eng.set_option("mask_wide", 1)
    mixed, fresh = [a, fb, b, fa, a], [fa, fb, fb, fa, fa]
    assert _hits(vb.fuzzy_lookup_embeddings_scoped(qs[:5], mixed, 10, 0.0)) == _hits(vb.fuzzy_lookup_embeddings_scoped(qs[:5], fresh, 10, 0.0))
    both = a & fb
    assert both.count == int((a1 & b1).sum())
    assert_same_handle(both, vb.row_mask(a1 & b1))
    # the row -> message map shrank with the removal
    assert np.array_equal(vb._row_messages, msgs[~gone])
    got = vb.lookup_messages_by_embedding_masked(qs[1], a, 5, 0.0)
    want = vb.lookup_messages_by_embedding_masked(qs[1], fa, 5, 0.0)
    assert [(m.item, m.score) for m in got] == [(m.item, m.score) for m in want] and len(got) > 0


# ---- a sequence of edits --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", mc.DTYPES)
def test_an_edit_sequence_carries_its_handles_across_every_step(dtype):
    n = mc.CHUNK + 3000  # (stays beyond one chunk through every step)
    base = mc.base_matrix()
    vb = new_vb(base[:n], dtype)
    rng = np.random.default_rng(5)
    bools = [rng.random(n) < 0.5, np.arange(n) % 7 == 0, np.arange(n) >= n - 100]
    handles = [vb.row_mask(b) for b in bools]
    left = vb.row_mask(np.ones(n, dtype=bool))  # not carried

    def check(step):
        for i, (h, b) in enumerate(zip(handles, bools)):
            assert len(b) == len(vb)
            assert_same_handle(h, vb.row_mask(b), f"{step} mask {i}")

    gone = rng.random(n) < 0.1
    assert vb.remove_rows(gone, carry=handles) == int(gone.sum())
    bools = [b[~gone] for b in bools]
    check("remove")
    with pytest.raises(ValueError, match="covers"):  # (the length is checked first; at the old length again it is the epoch: below)
        vb.fuzzy_lookup_embedding_masked(base[0], left, 3, 0.0)
    vb.add_embeddings(None, np.array(base[n : n + 33]))
    with pytest.raises(ValueError, match="covers"):
        vb.fuzzy_lookup_embedding_masked(base[0], handles[0], 3, 0.0)
    vb.extend_masks(*handles, new=True)
    bools = [np.concatenate([b, np.ones(33, dtype=bool)]) for b in bools]
    check("append")
    at = np.array([0, 5, 5, len(vb), mc.CHUNK - 1, mc.CHUNK - 1])
    assert vb.insert_rows(at, np.array(base[n + 33 : n + 39]), carry=handles) == 6
    bools = [np.insert(b, at, False) for b in bools]
    check("insert")
    assert vb.set_rows([0, 1, len(vb) - 1], np.array(base[n + 40 : n + 43])) == 3
    check("set_rows")
    assert vb.remove_rows(handles[1], carry=handles) == int(bools[1].sum())
    bools = [b[~bools[1]] for b in bools]
    assert handles[1].count == 0
    check("remove by a handle")
    vb.add_embeddings(None, np.array(base[: n - len(vb)]))
    assert len(vb) == n == left.rows
    with pytest.raises(ValueError, match="removed from"):
        vb.fuzzy_lookup_embedding_masked(base[0], left, 3, 0.0)
    vb.extend_masks(*handles)
    assert len(vb.fuzzy_lookup_embedding_masked(base[0], handles[0], 3, 0.0)) == 3


def test_a_device_only_corpus_stays_on_the_device_under_carried_edits(monkeypatch):
    n = 5000
    base = mc.base_matrix()
    vb = new_vb(base[:n], "fp16", keep_host_copy=False)
    assert vb._device_only is not None
    monkeypatch.setattr(vb, "_materialize_host", lambda: pytest.fail("a carried edit copied a device-only corpus to the host"))
    b = np.arange(n) % 5 == 0
    h = vb.row_mask(b)
    monkeypatch.setattr(vb, "_mask_bools", lambda mask: pytest.fail("the device route read a carried mask back"))
    flags = np.arange(n) % 7 == 3
    assert vb.remove_rows(flags, carry=[h]) == int(flags.sum())
    b = b[~flags]
    assert vb.insert_rows([1, 1, 700], np.array(base[n : n + 3]), carry=[h], carry_new=True) == 3
    b = np.insert(b, [1, 1, 700], True)
    vb.add_embeddings(None, np.array(base[n + 3 : n + 8]))
    vb.extend_masks(h)
    b = np.concatenate([b, np.zeros(5, dtype=bool)])
    assert vb._device_only is not None and vb._device_only is vb._engine.corpus and vb._host.shape[0] == 0
    monkeypatch.undo()
    assert_same_handle(h, vb.row_mask(b))
    assert vb._device_only is not None
