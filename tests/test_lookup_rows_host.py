"""CPU suite: `VectorBase.fuzzy_lookup_rows` and `near_duplicate_pairs` on a host-only index (the numpy engine of tests/fake_engine.py: the
class takes its host route, which is the methods' definition), over the table of tests/lookup_rows_cases.py.

  * the table names its branches, every required name has a case, and every case reaches what it is in the table for;
  * per row, `fuzzy_lookup_rows` equals the reference statement -- `fuzzy_lookup_embedding(vectors[i], max_hits + 1, min_score)` with the entry
    `item == i` removed, cut to max_hits -- through the oracle: items exact, scores within 1e-5, near-ties decided by the float64 referee;
  * the ordinal rules are numpy's: negatives wrap, duplicates are answered twice, out of range raises IndexError, an empty list gives an
    empty list, an int is a list of one;
  * `near_duplicate_pairs` equals the definition loop exactly and a float64 brute force outside near-ties, with and without `among`;
  * the entry points are declared, bound and exported, refuse bad arguments without a GPU, and their options are documented."""

import ctypes
import os

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests import lookup_rows_cases as lc
from tests.fake_engine import FakeEngine
from tests.fakes import NullModel
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native, adapters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tavb_search_rows", "tavb_search_rows_device", "tavb_search_rows_sorted", "tavb_gather_rows_f32")
IDS = [c.name for c in lc.CASES]


def host_index(monkeypatch, v: np.ndarray, dtype: str = "fp32") -> VectorBase:
    monkeypatch.setattr(_native, "Engine", FakeEngine)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=dtype)
    vb.add_embeddings(None, np.array(v))
    return vb


def check_row(v: np.ndarray, i: int, hits, max_hits: int, min_score: float, exclude_self: bool = True) -> None:
    """`hits` against the reference statement for row i"""
    items, scores = [h.item for h in hits], [h.score for h in hits]
    with np.errstate(invalid="ignore", over="ignore"):
        ref = vo.lookup(v, v[i], (max_hits + 1 if exclude_self else max_hits) if max_hits else 0, min_score)
    if exclude_self:
        ref = [(o, s) for o, s in ref if o != i]
    ref = ref[:max_hits] if max_hits else ref
    if items == [o for o, _ in ref]:
        assert len(scores) == len(ref) and all(abs(a - b) <= vo.SCORE_TOL for a, (_, b) in zip(scores, ref))
        return
    # a near-tie (the planted duplicates score alike): the float64 referee over the rows the lookup may return
    others = np.array([j for j in range(len(v)) if j != i or not exclude_self], dtype=np.int64)
    vo.check_topk_parity(vo.scores_full(v[others], v[i]), items, scores, max_hits, min_score, candidate_ordinals=others,
                         referee=vo.f64_referee(v[others], v[i]))


def test_table_is_what_the_suite_is_for():
    assert len(IDS) == len(set(IDS)) and len(lc.CASES) == 30
    hit = set()
    for c in lc.CASES:
        hit |= lc.branches(c)
    assert lc.REQUIRED <= hit, f"no case for {sorted(lc.REQUIRED - hit)}"
    assert {c.corpus.dim for c in lc.CASES} == {64, 100, 1536} and {c.corpus.dtype for c in lc.CASES} == {"fp32", "fp16"}
    for c in lc.CORPORA:
        assert 700 <= c.rows <= 2600 and lc.big_group(c)[-1] < c.rows
        v = lc.vectors(c)
        g = lc.big_group(c)
        assert (v[g] == v[g[0]]).all() and not v[lc.ZERO_ROW].any() and abs(np.linalg.norm(v[lc.NORM3_ROW]) - 3.0) < 1e-2
    # the member of the big group with the highest ordinal is not in its own k + 1 list for every k the group is built for
    c = lc.SMALL32
    v, last = lc.vectors(c), int(lc.big_group(c)[-1])
    top = vo.lookup(v, v[last], 11, 0.0)
    assert len(top) == 11 and all(s == top[0][1] for _, s in top)
    assert {e[0] for e in lc.EDGE_CASES} >= {"negative", "duplicate-ordinal", "out-of-range", "empty", "int"}


@pytest.mark.parametrize("case", lc.CASES, ids=IDS)
def test_fuzzy_lookup_rows_equals_the_reference_statement(monkeypatch, case):
    c = case.corpus
    v = lc.vectors(c)
    vb = host_index(monkeypatch, v, c.dtype)
    asked = lc.ordinals(c, case.n)
    got = vb.fuzzy_lookup_rows(asked, case.max_hits, case.min_score)
    assert len(got) == len(asked)
    for r in sorted(set(range(min(len(asked), 12))) | {len(asked) - 1}):  # the planted rows lead the list
        i = asked[r] + c.rows if asked[r] < 0 else asked[r]
        assert all(h.item != i for h in got[r]), f"{case.name}: row {i} is in its own list"
        if case.max_hits:
            assert len(got[r]) <= case.max_hits
        check_row(v, i, got[r], case.max_hits, case.min_score)
    if "self-below-min-score" in lc.branches(case):
        assert got[asked.index(lc.ZERO_ROW)] == []
    # a row asked twice is answered twice
    first = {}
    for r, o in enumerate(asked):
        i = o + c.rows if o < 0 else o
        if i in first:
            assert got[r] == got[first[i]]
        first.setdefault(i, r)


def test_exclude_self_false_is_the_plain_lookup(monkeypatch):
    c = lc.SMALL32
    v = lc.vectors(c)
    vb = host_index(monkeypatch, v)
    asked = lc.ordinals(c, 9)
    pos = [o + c.rows if o < 0 else o for o in asked]
    for max_hits in (1, 10, 300, 0):
        got = vb.fuzzy_lookup_rows(asked, max_hits, 0.3, exclude_self=False)
        assert got == vb.fuzzy_lookup_embeddings(v[pos], max_hits, 0.3)
        assert got[3][0].item in lc.PAIR  # a unit row is its own best match (with its copy)


def test_ordinal_rules_are_numpys(monkeypatch):
    c = lc.SMALL32
    v = lc.vectors(c)
    vb = host_index(monkeypatch, v)
    for name, ords, want in lc.EDGE_CASES:
        if want == "IndexError":
            with pytest.raises(IndexError):
                vb.fuzzy_lookup_rows(ords, 5)
            continue
        got = vb.fuzzy_lookup_rows(ords, 5, 0.0)
        if want == "empty":
            assert got == []
        elif want == "one":
            assert len(got) == 1 and got == vb.fuzzy_lookup_rows([ords], 5, 0.0)
            check_row(v, ords, got[0], 5, 0.0)
        elif want == "twice":
            assert len(got) == len(ords) and all(g == got[0] for g in got)
        else:
            assert got == vb.fuzzy_lookup_rows([int(o) % c.rows for o in ords], 5, 0.0), name
    # defaults come from the settings' rules, as in fuzzy_lookup_embeddings: 10 hits, every score
    assert len(vb.fuzzy_lookup_rows([3])[0]) == 10
    with pytest.raises(IndexError):
        vb.fuzzy_lookup_rows([0.5], 5)
    with pytest.raises(ValueError):
        vb.fuzzy_lookup_rows([1], -1)
    empty = VectorBase(TextEmbeddingIndexSettings(NullModel()))
    assert empty.fuzzy_lookup_rows([]) == []
    with pytest.raises(IndexError):
        empty.fuzzy_lookup_rows([0])


def _f64_pairs(v: np.ndarray, min_score: float, max_per_row: int, allowed):
    """float64 brute force: per row i the admissible j > i scoring at least min_score, best first"""
    out = {}
    v64 = v.astype(np.float64)
    for i in range(len(v)):
        if allowed is not None and not allowed[i]:
            continue
        s = np.clip((v64[i + 1:] @ v64[i] + 1.0) / 2.0, 0.0, 1.0)
        js = np.arange(i + 1, len(v))
        ok = s >= min_score - 4 * vo.TIE_EPS
        if allowed is not None:
            ok &= allowed[i + 1:]
        out[i] = (js[ok], s[ok])
    return out


@pytest.mark.parametrize("with_among", [False, True], ids=["all-rows", "among"])
@pytest.mark.parametrize("max_per_row", [1, 2, 16])
def test_near_duplicate_pairs_equals_the_definition_and_a_float64_brute_force(monkeypatch, with_among, max_per_row):
    v = lc.pairs_corpus()
    vb = host_index(monkeypatch, v)
    allowed = lc.among_mask(len(v)) if with_among else None
    min_score = 0.97
    i, j, s = vb.near_duplicate_pairs(min_score, max_per_row, among=allowed)
    assert i.dtype == np.int64 and j.dtype == np.int64 and s.dtype == np.float32 and len(i) == len(j) == len(s)
    assert (i < j).all() and len(set(zip(i.tolist(), j.tolist()))) == len(i)
    if not with_among and max_per_row == 16:
        assert 140 <= len(i) <= 260  # about 150 planted pairs, the triples' extra pairs
    # sorted by (i, score descending, j ascending)
    assert np.array_equal(np.lexsort((j, -s.astype(np.float64), i)), np.arange(len(i)))

    def lookup_all(row):
        hits = vb.fuzzy_lookup_embedding(v[row], max_hits=0, min_score=min_score)
        return [h.item for h in hits], [h.score for h in hits]

    want = lc.definition_pairs(lookup_all, len(v), min_score, max_per_row, allowed)
    assert list(zip(i.tolist(), j.tolist(), s.tolist())) == want
    # the float64 brute force: every pair is one of its pairs, and per row nothing clearly better was left out
    truth = _f64_pairs(v, min_score, max_per_row, allowed)
    width = 8 * vo.TIE_EPS
    by_row = {}
    for a, b, sc in zip(i.tolist(), j.tolist(), s.tolist()):
        by_row.setdefault(a, []).append((b, sc))
    for a, (js, ss) in truth.items():
        got = by_row.get(a, [])
        t = dict(zip(js.tolist(), ss.tolist()))
        for b, sc in got:
            assert b in t and abs(t[b] - sc) <= vo.SCORE_TOL
        sure = ss >= min_score + 4 * vo.TIE_EPS
        assert len(got) >= min(max_per_row, int(sure.sum())), (a, got)
        if got and len(got) == max_per_row:
            left = [t[b] for b in js.tolist() if b not in {g[0] for g in got}]
            assert not left or max(left) <= min(t[b] for b, _ in got) + width
    if with_among:
        assert allowed[i].all() and allowed[j].all()


def test_near_duplicate_pairs_widens_its_lookups_until_every_row_is_settled(monkeypatch):
    """A cluster of 40 copies and max_per_row = 2: for the cluster's LAST rows the few best others all have lower ordinals, so the first
    lookups hold no admissible j; the method asks again with more hits and finds the pairs behind."""
    rng = np.random.default_rng(3)
    v = rng.standard_normal((300, 32)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    cluster = np.arange(40) * 3 + 50
    v[cluster] = v[cluster[0]]
    vb = host_index(monkeypatch, v)
    i, j, s = vb.near_duplicate_pairs(0.99, 2)
    want = [(int(a), int(b)) for n_, a in enumerate(cluster) for b in cluster[n_ + 1:n_ + 3]]
    assert list(zip(i.tolist(), j.tolist())) == want and (s == s[0]).all()
    assert vb.near_duplicate_pairs(1.5, 2)[0].size == 0
    with pytest.raises(ValueError):
        vb.near_duplicate_pairs(0.9, 0)


def test_find_duplicate_terms_names_the_pairs(monkeypatch):
    v = lc.pairs_corpus()[:200].copy()
    v[150] = v[3]
    v[199] = v[3]
    vb = host_index(monkeypatch, v)
    texts = [f"term{n}" for n in range(len(v))]

    class MemoryIndex:
        _vectorbase, _texts = vb, texts

    class SqliteIndex:
        _vector_base, _terms_list = vb, texts

    for index in (MemoryIndex(), SqliteIndex()):
        pairs = adapters.find_duplicate_terms(index, 0.999)
        assert [p[:2] for p in pairs if p[0] == "term3"] == [("term3", "term150"), ("term3", "term199")]
        assert ("term150", "term199") in [p[:2] for p in pairs] and all(isinstance(p[2], float) and p[2] >= 0.999 for p in pairs)
    with pytest.raises(TypeError):
        adapters.find_duplicate_terms(object(), 0.9)


def test_entry_points_are_declared_bound_exported_and_refuse_bad_arguments():
    text = open(os.path.join(ROOT, "include", "tavb.h")).read()
    lib = _native.load_library(preload_torch=False)
    for name in NEW:
        assert f"int {name}(" in text and name in _native.ABI_SYMBOLS and hasattr(lib, name), name
    for name in ("rows_query", "rows_query_wave", "rows_query_launches"):
        assert f'"{name}"' in text, name
    total = ctypes.c_int64(0)
    assert lib.tavb_search_rows(None, None, 1, 10, 1, None, None, None, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_rows_device(None, None, 1, 10, 1, None, None, None) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_search_rows_sorted(None, None, 1, 1, None, 0, None, None, None, ctypes.byref(total)) == -1 and b"null context" in lib.tavb_last_error()
    assert lib.tavb_gather_rows_f32(None, None, 1, None) == -1 and b"null context" in lib.tavb_last_error()


def test_route_predicate():
    class Opt:
        def __init__(self, on):
            self.on = on

        def get_option(self, name):
            assert name == "rows_query"
            return self.on

    class Eng(Opt, _native.Engine):  # an Engine in type only (no device is opened)
        def __init__(self, on):
            Opt.__init__(self, on)

    assert VectorBase._rows_native(Eng(1)) and not VectorBase._rows_native(Eng(0))
    assert not VectorBase._rows_native(Opt(1)) and not VectorBase._rows_native(FakeEngine())
