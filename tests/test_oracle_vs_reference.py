"""CPU suite: the numpy oracle and the host side of the new class against what the VERBATIM reference class returns.
The reference's answers are stored in tests/golden/reference_answers.json, written by tests/golden/make_reference_answers.py
(which executes the reference's vectorbase.py and aitools/embeddings.py unmodified through oracle/ref_loader.py); the inputs
are regenerated here from their seeds, and the observations are made by the same functions on both sides."""

import asyncio
import json
import os

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_NS = [(1, 1), (7, 3), (300, 17), (1000, 384), (5000, 1536)]
FULL_KS = [None, 1, 10, 32, 50]
FULL_MIN_SCORES = [None, 0.0, 0.5, 0.53, 0.85, 1.0, 1.5]
SMALL_KS = (41, 1000, 0)
SMALL_SUBSETS = ([3, 3, 1, 0], [-1, 5], list(range(40)), [39])
COSINES = np.linspace(-1.5, 1.5, 101, dtype=np.float32)


@pytest.fixture(scope="module")
def answers():
    with open(os.path.join(ROOT, "tests", "golden", "reference_answers.json")) as f:
        return json.load(f)


def _pairs(res):
    return [(int(r.item), float(r.score)) for r in res]


def _stored(pairs):
    return [(int(i), float(s)) for i, s in pairs]


def full_case(n: int, d: int):
    rng = np.random.default_rng(n * 1000 + d)
    v = rng.standard_normal((n, d)).astype(np.float32)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    q = v[rng.integers(n)] * 0.8 + 0.2 * rng.standard_normal(d).astype(np.float32)
    q = (q / np.linalg.norm(q)).astype(np.float32)
    return v, q


def full_key(n, d, k, min_score) -> str:
    return f"{n},{d},{k},{min_score}"


def small_case():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((40, 6)).astype(np.float32)
    q = rng.standard_normal(6).astype(np.float32)
    return v, q


def small_predicate(i):
    return i % 3 == 1


def bookkeeping_observations(vb) -> dict:
    """The same sequence of host-side calls on an empty VectorBase: lengths, matrices and the errors it raises."""
    rng = np.random.default_rng(2)
    a = rng.standard_normal((5, 4)).astype(np.float32)
    obs = {"empty": [len(vb), bool(vb), list(vb.serialize().shape)]}
    vb.add_embedding(None, a[0])
    vb.add_embedding(None, list(map(float, a[1])))
    vb.add_embeddings(None, a[2:])
    m = vb.serialize()
    obs["filled"] = [len(vb), int(vb._embedding_size), str(m.dtype), list(m.shape), m.tolist()]
    errors = []
    for call in (lambda: vb.add_embedding(None, np.zeros(2, dtype=np.float32)), lambda: vb.add_embeddings(None, np.zeros((1, 1, 4), dtype=np.float32)),
                 lambda: vb.get_embedding_at(5)):
        try:
            call()
            errors.append(None)
        except Exception as exc:  # noqa: BLE001 -- the type and message are what is compared
            errors.append([type(exc).__name__, str(exc)])
    obs["errors"] = errors
    obs["serialize_embedding_at_-1"] = repr(vb.serialize_embedding_at(-1))
    vb.clear()
    obs["cleared"] = [len(vb), list(vb.serialize().shape)]
    return obs


CACHING_SCRIPT = [("one", "a"), ("many", ["a", "bb", "bb", "ccc"]), ("one", "bb"), ("many", ["dddd"]), ("many", ["a", "dddd"]), ("one", "zz"),
                  ("many", ["zz", "yy", "yy"]), ("add", "pre"), ("one", "pre"), ("many", ["pre", "q"])]


def caching_observations(cls) -> dict:
    """The calls a CachingEmbeddingModel class makes on a counting embedder over CACHING_SCRIPT, what it returns, what it caches."""

    class Counting:
        model_name = "counting"

        def __init__(self):
            self.calls = []

        async def get_embedding_nocache(self, input):
            self.calls.append(["one", input])
            return np.full(3, float(len(input)), dtype=np.float32)

        async def get_embeddings_nocache(self, input):
            self.calls.append(["many", list(input)])
            return np.stack([np.full(3, float(len(s)), dtype=np.float32) for s in input])

    emb = Counting()
    model = cls(emb)
    outs = []
    for op, arg in CACHING_SCRIPT:
        if op == "one":
            out = asyncio.run(model.get_embedding(arg))
        elif op == "many":
            out = asyncio.run(model.get_embeddings(arg))
        else:
            model.add_embedding(arg, np.full(3, 9.0, dtype=np.float32))
            continue
        outs.append([str(out.dtype), list(out.shape), out.tolist()])
    try:
        asyncio.run(cls(Counting()).get_embeddings([]))
        empty = None
    except Exception as exc:  # noqa: BLE001
        empty = type(exc).__name__
    return {"calls": emb.calls, "outs": outs, "cache_keys": sorted(model._cache), "empty_batch_raises": empty}


@pytest.mark.parametrize("n,d", FULL_NS)
@pytest.mark.parametrize("k", FULL_KS)
@pytest.mark.parametrize("min_score", FULL_MIN_SCORES)
def test_full_lookup_differential(n, d, k, min_score, answers):
    v, q = full_case(n, d)
    assert vo.lookup(v, q, k, min_score) == _stored(answers["full_lookup"][full_key(n, d, k, min_score)])


def test_k_larger_than_n_and_zero_quirk_and_subset_and_predicate(answers):
    ref = answers["small"]
    v, q = small_case()
    for k in SMALL_KS:
        assert vo.lookup(v, q, k, 0.0) == _stored(ref["k"][str(k)])
    for sub, want in zip(SMALL_SUBSETS, ref["subsets"]):
        assert vo.lookup_in_subset(v, q, sub, 5, 0.0) == _stored(want)
    assert ref["subset_out_of_range_raises"] == "IndexError"
    with pytest.raises(IndexError):
        vo.lookup_in_subset(v, q, [40], 5, 0.0)
    assert vo.lookup(v, q, 4, 0.2, small_predicate) == _stored(ref["predicate"])


def test_cosine_to_score_and_settings_match(answers):
    ref = answers["scores_and_settings"]
    want = np.asarray(ref["cosine_to_score"], dtype=ref["cosine_to_score_dtype"])
    np.testing.assert_array_equal(vo.cosine_to_score(COSINES), want)
    from typeagent_py_amd import vectorbase as mine

    got = mine.cosine_to_score(COSINES)
    assert str(np.asarray(got).dtype) == ref["cosine_to_score_dtype"]
    np.testing.assert_array_equal(got, want)
    assert mine.MODEL_DEFAULT_MIN_SCORES == ref["MODEL_DEFAULT_MIN_SCORES"]
    assert mine.DEFAULT_MIN_SCORE == ref["DEFAULT_MIN_SCORE"]
    for name, score in ref["get_default_min_score"].items():
        assert mine.get_default_min_score(name) == score
    assert "other" in ref["get_default_min_score"] and set(ref["MODEL_DEFAULT_MIN_SCORES"]) < set(ref["get_default_min_score"])


def test_host_side_class_matches_reference_bookkeeping(answers):
    """Same sequence of host-side calls on both classes -> same lengths, matrices and errors."""
    from tests.fakes import NullModel
    from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase

    mine = bookkeeping_observations(VectorBase(TextEmbeddingIndexSettings(embedding_model=NullModel())))
    assert json.loads(json.dumps(mine)) == answers["bookkeeping"]
    assert mine["empty"] == [0, True, [0]] and mine["filled"][:2] == [5, 4] and mine["cleared"] == [0, [0, 4]]
    assert mine["errors"] == [["ValueError", "Embedding size mismatch: expected 4, got 2"], ["ValueError", "Expected 2D embeddings array, got 3D"],
                              ["IndexError", "Index 5 out of bounds for embedding index of size 5"]]
    assert mine["serialize_embedding_at_-1"] == "None"


def test_caching_embedding_model_makes_the_reference_calls(answers):
    """`CachingEmbeddingModel` is registered as typeagent.aitools.embeddings' class by install(): embedders that count, log or bill their
    calls -- and batch-only ones -- must see the call pattern of the reference's class (aitools/embeddings.py:73-114), recorded in the
    golden file together with what it returned and cached."""
    from typeagent_py_amd.embeddings import CachingEmbeddingModel

    mine = caching_observations(CachingEmbeddingModel)
    assert json.loads(json.dumps(mine)) == answers["caching_embedding_model"]
    assert mine["cache_keys"] == sorted({"a", "bb", "ccc", "dddd", "zz", "yy", "pre", "q"}) and mine["empty_batch_raises"] == "ValueError"
