#!/usr/bin/env python3
"""Generate tests/golden/reference_answers.json from the VERBATIM reference.

Needs a checkout of the reference project (oracle/ref_loader.py: TAVB_REFERENCE_ROOT):

    python tests/golden/make_reference_answers.py

Every answer in the JSON comes from the reference's own code -- `VectorBase`, `cosine_to_score` and the settings table of
src/typeagent/aitools/vectorbase.py, `CachingEmbeddingModel` of src/typeagent/aitools/embeddings.py, executed unmodified
(embeddings.py with its two PEP 695 `type X = ...` alias statements rewritten as plain assignments, nothing else touched) --
over the inputs and through the observation functions of tests/test_oracle_vs_reference.py and tests/test_host_api.py, which
compare the oracle and the new class against it.
"""

from __future__ import annotations

import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_loader  # noqa: E402
from tests import test_host_api as th  # noqa: E402
from tests import test_oracle_vs_reference as tv  # noqa: E402
from tests.fakes import NullModel  # noqa: E402


def _pairs(res):
    return [[int(r.item), float(r.score)] for r in res]


def reference_embeddings_module():
    path = os.path.join(ref_loader.REFERENCE_ROOT, "src", "typeagent", "aitools", "embeddings.py")
    src = open(path).read()
    new_src, n_changed = re.subn(r"(?m)^type (\w+) = ", r"\1 = ", src)
    assert n_changed == 2 and len(new_src.splitlines()) == len(src.splitlines())
    mod = types.ModuleType("ref_embeddings")
    exec(compile(new_src, path, "exec"), mod.__dict__)
    return mod


def main() -> None:
    mod = ref_loader.load_reference_vectorbase()
    out = {"full_lookup": {}}
    for n, d in tv.FULL_NS:
        v, q = tv.full_case(n, d)
        ref = ref_loader.make_reference_vectorbase(v)
        for k in tv.FULL_KS:
            for ms in tv.FULL_MIN_SCORES:
                out["full_lookup"][tv.full_key(n, d, k, ms)] = _pairs(ref.fuzzy_lookup_embedding(q, max_hits=k, min_score=ms))

    v, q = tv.small_case()
    ref = ref_loader.make_reference_vectorbase(v)
    small = {"k": {str(k): _pairs(ref.fuzzy_lookup_embedding(q, max_hits=k, min_score=0.0)) for k in tv.SMALL_KS},
             "subsets": [_pairs(ref.fuzzy_lookup_embedding_in_subset(q, sub, max_hits=5, min_score=0.0)) for sub in tv.SMALL_SUBSETS],
             "predicate": _pairs(ref.fuzzy_lookup_embedding(q, max_hits=4, min_score=0.2, predicate=tv.small_predicate))}
    try:
        ref.fuzzy_lookup_embedding_in_subset(q, [40], max_hits=5, min_score=0.0)
        small["subset_out_of_range_raises"] = None
    except Exception as exc:  # noqa: BLE001
        small["subset_out_of_range_raises"] = type(exc).__name__
    out["small"] = small

    c2s = np.asarray(mod.cosine_to_score(tv.COSINES))
    out["scores_and_settings"] = {
        "cosine_to_score": c2s.tolist(), "cosine_to_score_dtype": str(c2s.dtype),
        "MODEL_DEFAULT_MIN_SCORES": dict(mod.MODEL_DEFAULT_MIN_SCORES), "DEFAULT_MIN_SCORE": mod.DEFAULT_MIN_SCORE,
        "get_default_min_score": {name: mod.get_default_min_score(name) for name in list(mod.MODEL_DEFAULT_MIN_SCORES) + ["other"]},
    }
    out["bookkeeping"] = tv.bookkeeping_observations(mod.VectorBase(mod.TextEmbeddingIndexSettings(embedding_model=NullModel())))
    out["caching_embedding_model"] = tv.caching_observations(reference_embeddings_module().CachingEmbeddingModel)
    out["scored_int"] = th.scored_int_observations(mod.ScoredInt)

    path = os.path.join(HERE, "reference_answers.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {path}: {len(out['full_lookup'])} full lookups, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
