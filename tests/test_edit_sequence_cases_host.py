"""CPU suite: the case table of tests/edit_sequence_cases.py without a GPU.  The table is complete (every corpus kind x every edit step kind x
every route leg the kind has occurs, so a deleted case fails); every sequence replayed on a host-only `VectorBase` (the suite's engine double:
the class takes its host route) ends in the table's numpy model bit for bit, row -> message map included; and by the oracle's float64 scores
every query of a non-planted leg leaves more than GAP between rank k and rank k + 1 -- and between the row it is aimed at and rank 2 -- so no
comparison of tests/test_gpu_edit_sequences.py can be forgiven as a tie.  The planted leg goes through the referee, which forgives swaps only
inside the cluster: its near-ties are cluster rows, which the last test shows."""

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import edit_sequence_cases as ec
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native


@pytest.fixture
def fake(monkeypatch):
    from typeagent_py_amd import multidevice

    monkeypatch.setattr(_native, "Engine", FakeEngine)
    monkeypatch.setattr(multidevice._native, "Engine", FakeEngine)


def test_the_table_is_the_whole_product():
    assert ec.CHUNK == _native.MASK_ROWS_PER_WORKGROUP and ec.ROWS == ec.CHUNK + 1
    assert [(k.dtype, k.dim, k.shadow, k.tile) for k in ec.KINDS] == [("fp32", 128, 1, True), ("fp16", 100, 1, False), ("fp16", 72, 1, False), ("fp16", 128, 0, True)]
    assert len(ec.CASES) == 88 and len({c.id for c in ec.CASES}) == len(ec.CASES)
    assert {leg.name for leg in ec.LEGS} == {"single", "tile32", "tile64", "shadow-tile", "wide128", "wide256", "flagged", "masked-gather", "masked-tile32",
                                             "masked-tile64", "masked-wide", "scoped", "large-k", "sort-all", "messages", "messages-scoped"}
    # the legs a kind does not have, spelled out: the 32/64-query tile needs rows of whole 64-byte steps, the shadow tile an fp32 corpus, the masked
    # wide tile an fp16 one
    missing = {k.name: {leg.name for leg in ec.LEGS} - {leg.name for leg in ec.legs_of(k)} for k in ec.KINDS}
    tiles = {"tile32", "tile64", "masked-tile32", "masked-tile64"}
    assert missing == {"f32-d128": {"masked-wide"}, "f16-d100": tiles | {"shadow-tile"}, "f16-d72": tiles | {"shadow-tile"}, "f16-d128": {"shadow-tile"}}
    for leg in ec.LEGS:
        assert leg.name == "messages" or leg.expect, f"{leg.name} names no route"
        assert leg.k in (0, 8, 25, 32, 300) and (leg.nq <= ec.NQ)
    assert ec.LEG["large-k"].k == 300 and ec.LEG["sort-all"].k == 0 and ec.LEG["scoped"].nq == 8 and {ec.LEG["wide128"].k, ec.LEG["wide256"].k} == {8, 32}
    for kind in ec.KINDS:
        for p in ec.PASSES:
            seen = {s.kind for c in ec.CASES if c.kind == kind and c.pass_rows == p for s in c.sequence.steps if s.lookups or s.op == "append"}
            want = set(ec.STEP_KINDS) if p == 0 else {sk for sk in ec.STEP_KINDS if sk[0] in ("insert", "remove")}
            assert seen >= want, (kind.name, p, want - seen)
        # every step kind is followed by every leg of the kind: a checkpoint runs all of them (the append also without a lookup: the cold tail)
        assert any(not s.lookups and s.op == "append" for c in ec.CASES if c.kind == kind for s in c.sequence.steps)
        assert any(not c.sequence.keep_host_copy for c in ec.CASES if c.kind == kind)
    # the product itself: every (kind, step kind, leg of the kind) is a checkpoint leg of some case -- at the default passes, and for the steps
    # that move rows in place under short passes as well
    for p in ec.PASSES:
        have = {(c.kind.name, s.kind, leg.name) for c in ec.CASES if c.pass_rows == p for s in c.sequence.steps if s.lookups for leg in ec.legs_of(c.kind)}
        steps = [sk for sk in ec.STEP_KINDS if p == 0 or sk[0] in ("insert", "remove")]
        want = {(k.name, sk, leg.name) for k in ec.KINDS for sk in steps for leg in ec.legs_of(k)}
        assert want <= have, sorted(want - have)[:5]
        assert len(want) == sum(len(ec.legs_of(k)) for k in ec.KINDS) * len(steps)
    names = [s.name for s in ec.SEQUENCES]
    assert names[-2:] == ["long", "long-device-only"] and [s.op for s in ec.LONG] == ["remove", "append", "insert", "set", "remove"]


@pytest.mark.parametrize("kind", ec.KINDS, ids=[k.name for k in ec.KINDS])
def test_sequences_on_a_host_only_index_end_in_the_model_and_every_query_has_its_gap(fake, kind):
    aims, end_rows = set(), 0  # what the aimed queries cover over the kind's sequences
    for seq in ec.SEQUENCES:
        if not seq.keep_host_copy:
            continue  # (the same edits; the engine double keeps a host matrix)
        raw, msgs, _, _, _ = ec.base(kind)
        vb = VectorBase(TextEmbeddingIndexSettings(NullModel()))
        vb.add_embeddings(None, raw[: ec.ROWS - 1].copy())
        vb.add_embeddings(None, raw[ec.ROWS - 1 :].copy())
        vb.set_row_messages(msgs)
        model = ec.start(kind)
        for i, (e, cp) in enumerate(ec.checkpoints(kind, seq.name)):
            what = f"{kind.name} {seq.name} step {i} ({e.step.op} {e.step.where})"
            # what the step's name promises about norm_rows
            nr = model.norm_rows
            if e.step.op == "set" or (e.step.op == "append") or e.first >= nr:
                assert e.norm_rows == nr and e.model.cap == model.cap, what
            else:
                assert e.norm_rows == 0, what
            if e.step.kind in (("insert", "tail"), ("set", "above"), ("set", "straddle"), ("remove", "across"), ("remove", "after")):
                assert 0 < nr < len(model), what  # a cold tail
            ec.apply_edit(vb, e)
            model = e.model
            assert len(vb) == len(model), what
            np.testing.assert_array_equal(np.asarray(vb.serialize()), model.raw, err_msg=what)
            np.testing.assert_array_equal(vb._row_messages[: len(model)], model.msgs, err_msg=what)
            assert int(model.tag.sum()) > 256 + 32, what  # the cluster still overflows a band of 256
            if cp is not None:
                check_gaps(kind, model, cp, what)
                aims |= {k for k, _ in cp.aimed}
                end_rows += sum(1 for k, r in cp.aimed if k == "moved" and r >= len(model) - 4)
    # new rows, moved rows (behind the edit and at the very end), rows in front and old contents all occur: what a stale cache would get wrong
    assert aims == {"new", "moved", "front", "old"} and end_rows >= 3, (kind.name, aims, end_rows)


def _scores64(v64, qs):
    return np.clip((v64 @ np.asarray(qs, dtype=np.float64).T + 1.0) / 2.0, 0.0, 1.0)


def _gaps64(s, k):
    top = -np.sort(np.partition(-s, k, axis=0)[: k + 1], axis=0)
    return top[k - 1] - top[k]


def check_gaps(kind, model, cp, what):
    v = ec.seen(kind, model.raw)
    v64 = v.astype(np.float64)
    flat = np.flatnonzero(cp.mask)
    for leg in ec.legs_of(kind):
        qs = ec.leg_queries(leg, cp)
        assert qs.shape == (leg.nq, kind.dim), (what, leg.name)
        if leg.planted:
            qs = qs[:-1]
        where = f"{what} leg {leg.name}"
        if leg.name == "sort-all":
            thr = ec.min_score_of(leg, kind)
            s = _scores64(v64, qs)
            assert np.abs(s - thr).min() > ec.GAP and ((s >= thr).sum(axis=0) >= 1).all(), where
        elif leg.call in ("scoped", "messages_scoped"):
            for qi, q in enumerate(qs):
                assert _gaps64(_scores64(v64[cp.scopes[qi]], q[None]), leg.k)[0] > ec.GAP, (where, qi)
        else:
            s = _scores64(v64[flat] if leg.call == "masked" else v64, qs)
            g = _gaps64(s, leg.k)
            assert g.min() > ec.GAP, (where, int(np.argmin(g)), float(g.min()))
    for qi, (kind_of, row) in enumerate(cp.aimed):
        s = vo.scores_f64(v, cp.queries[qi])
        if row >= 0:
            assert int(np.argmax(s)) == row and s[row] - np.delete(s, row).max() > ec.GAP, f"{what} aimed query {qi} ({kind_of})"
            assert cp.mask[row] and all(sc[row] for sc in cp.scopes)
    assert len(cp.aimed) >= 1 and {k for k, _ in cp.aimed} <= {"new", "moved", "front", "old"}, what


def test_the_planted_query_ties_only_with_its_cluster():
    """The flagged leg's last query: its best CLUSTER rows are the cluster (near-ties the referee may permute), and the gap to the best other
    row is far beyond GAP -- a swap the referee forgives is a swap inside the cluster."""
    for kind in ec.KINDS:
        raw, _, tag, c, _ = ec.base(kind)
        s = vo.scores_f64(ec.seen(kind, raw), c)
        order = np.argsort(-s)
        assert tag[order[: ec.CLUSTER]].all() and s[order[ec.CLUSTER - 1]] - s[order[ec.CLUSTER]] > 0.1
