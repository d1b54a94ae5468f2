"""CPU suite: FusedIndexQuery's result-buffer layout and its subset check, over the numpy stand-in engine (tests/fake_engine.py), which writes
nq x k keys at out_keys' first element, row q at q * k, as the kernels do -- and refuses, as the binding does, a buffer that cannot take them.
Also the binding's own out_keys check, on an Engine that never reaches the library."""

from __future__ import annotations

import contextlib

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.fake_engine import FakeEngine
from tests.synth import make_corpus, make_queries
from typeagent_py_amd import _native

torch = pytest.importorskip("torch")


class _Stream:
    def synchronize(self):
        pass


@pytest.fixture
def host_fused(monkeypatch):
    from typeagent_py_amd import fused

    monkeypatch.setattr(fused._native, "Engine", FakeEngine)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    monkeypatch.setattr(torch.cuda, "Stream", lambda d: _Stream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())

    def make(cls=fused.FusedIndexQuery):
        class Host(cls):
            def _alloc(self, nq, dim, n_keys):  # (plain host tensors for the pinned and the device buffers)
                return torch.empty((nq, dim)), torch.empty((nq, dim)), torch.zeros(n_keys, dtype=torch.int64)

        fq = Host(0)
        calls = []
        eng = fq.engine
        for name in ("search_device", "search_subset_device"):
            fn = getattr(eng, name)
            setattr(eng, name, lambda *a, _fn=fn, _n=name, **kw: (calls.append(_n), _fn(*a, **kw))[1])
        fq.calls = calls
        return fq

    return make


def _corpora(fq):
    t, _ = make_corpus(600, 64, 31)
    m, _ = make_corpus(400, 64, 32)
    h, _ = make_corpus(100, 64, 33)
    for name, v in (("terms", t), ("messages", m), ("threads", h)):
        fq.set_corpus(name, torch.from_numpy(v))
    return t, m, h


def _items(hits):
    return [x.item for x in hits]


def _oracle(v, q, k, ms, subset=None):
    sc = vo.scores_full(v, q) if subset is None else vo.scores_full(v[subset], q)
    ok = np.flatnonzero(sc >= np.float32(ms))
    order = ok[np.lexsort((ok, -sc[ok].astype(np.float64)))][:k]
    return order.tolist() if subset is None else [int(np.asarray(subset)[p]) for p in order]


def test_k_attributes_keep_every_list_in_its_rows(host_fused):
    """MESSAGES_K above TERMS_K (a subclass) and THREADS_K raised on an instance after a run of the same shape.  Before the fix the terms
    slice of the [nq, max K] buffer was strided (term lists landed in the wrong rows and were half zeroed), and the cached thread view was
    THREADS_K of the first run wide (the kernel wrote past the end of the pinned tensor)."""
    from typeagent_py_amd.fused import FusedIndexQuery

    class Wide(FusedIndexQuery):
        MESSAGES_K = 100
        THREADS_K = 60

    qs = make_queries(6, 64, 34)
    tq, mq, hq = qs[:4], qs[4], qs[5]
    for fq in (host_fused(Wide), host_fused()):
        t, m, h = _corpora(fq)
        if type(fq).__mro__[1] is FusedIndexQuery:
            fq.run(tq, mq, hq)
            fq.MESSAGES_K, fq.THREADS_K = 100, 60
        r = fq.run(tq, mq, hq)
        assert [_items(x) for x in r.terms] == [_oracle(t, q, 50, fq.TERMS_MIN) for q in tq]
        assert _items(r.messages) == _oracle(m, mq, 100, fq.MESSAGES_MIN)
        assert _items(r.threads) == _oracle(h, hq, 60, fq.THREADS_MIN)
        fq.TERMS_K = 3
        r = fq.run(tq, mq, hq)
        assert [_items(x) for x in r.terms] == [_oracle(t, q, 3, fq.TERMS_MIN) for q in tq]


def test_low_thresholds_fill_every_list(host_fused):
    """every list full (min_score 0): the three blocks do not overlap"""
    fq = host_fused()
    fq.TERMS_MIN = fq.MESSAGES_MIN = fq.THREADS_MIN = 0.0
    t, m, h = _corpora(fq)
    qs = make_queries(5, 64, 35)
    r = fq.run(qs[:3], qs[3], qs[4])
    assert [len(x) for x in r.terms] == [50] * 3 and len(r.messages) == 25 and len(r.threads) == 10
    assert [_items(x) for x in r.terms] == [_oracle(t, q, 50, 0.0) for q in qs[:3]]
    assert _items(r.messages) == _oracle(m, qs[3], 25, 0.0) and _items(r.threads) == _oracle(h, qs[4], 10, 0.0)
    sub = [5, -1, 5, 399, 0]
    r = fq.run(qs[:3], qs[3], qs[4], message_subset=sub)
    assert sorted(_items(r.messages)) == sorted(sub)


def test_bad_subset_raises_before_anything_is_enqueued(host_fused):
    fq = host_fused()
    _corpora(fq)
    qs = make_queries(6, 64, 36)
    good = fq.run(qs[:4], qs[4], qs[5])
    n_calls = len(fq.calls)
    for bad in ([0, 400], [-401], [3, 10_000]):
        with pytest.raises(IndexError):
            fq.run(qs[:4], qs[4], qs[5], message_subset=bad)
        assert len(fq.calls) == n_calls  # no lookup was enqueued
    assert fq.run(qs[:4], qs[4], qs[5]) == good


def _bare_engine():
    eng = _native.Engine.__new__(_native.Engine)
    eng._torch, eng.device, eng.dim = torch, 0, 8
    return eng


@pytest.mark.parametrize("make", [
    lambda: torch.zeros((4, 10), dtype=torch.int32),  # wrong dtype
    lambda: torch.zeros((4, 20), dtype=torch.int64)[:, :10],  # strided
    lambda: torch.zeros((3, 10), dtype=torch.int64),  # too small
    lambda: torch.zeros((4, 10), dtype=torch.int64),  # host memory that is not pinned
    lambda: np.zeros((4, 10), dtype=np.int64),  # not a tensor
])
def test_binding_refuses_an_out_keys_the_kernels_cannot_write(make):
    eng = _bare_engine()
    with pytest.raises(ValueError):
        eng._check_out_keys(make(), 4, 10)
