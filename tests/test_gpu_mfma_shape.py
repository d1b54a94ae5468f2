"""GPU suite: the 256-query filter tile on v_mfma_f32_16x16x32_f16 (option mfma_shape = 16, the default) against its 32x32x16 form.

The two shapes sum a filter score in different orders, so their filter scores differ in the last bits; the answers must not: the band is
complete by construction and every key that leaves the engine is rescored exactly.  Each case runs both shapes in one process on one corpus
and requires ordinals, score bits and counts to be identical, asserts through `last_mfma_shape` which kernel ran, and checks sampled queries
against the float64-refereed oracle as tests/test_gpu_routes.py does.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np
import pytest

from oracle import vectorbase_oracle as vo
from tests.synth import make_clustered_corpus, make_corpus, make_queries
from typeagent_py_amd import _native

pytestmark = pytest.mark.gpu

WIDE = (("direct_group_max_nq", 0),)


@dataclass(frozen=True)
class Case:
    name: str
    corpus: str  # "gauss", "clustered", "dup"
    dtype: str
    rows: int
    nq: int
    k: int
    opts: tuple = WIDE
    base: int = 0
    flagged: bool = False  # the early gate / split-plane fallback must run


CASES = [
    # 200_003 rows: not a multiple of the 320-row tile; the ladder runs several phases at this size (asserted below)
    Case("gauss-1024-k32", "gauss", "fp16", 200_003, 1024, 32),
    Case("gauss-1000-k1", "gauss", "fp16", 200_003, 1000, 1),
    Case("gauss-1000-k100", "gauss", "fp16", 200_003, 1000, 100),
    Case("gauss-1024-k256", "gauss", "fp16", 200_003, 1024, 256),
    Case("gauss-base-above-2^31", "gauss", "fp16", 200_003, 1024, 32, base=(1 << 31) + 12345),
    Case("clustered-1024-k32", "clustered", "fp16", 120_000, 1024, 32),
    # 1500-row clusters of near-duplicates with a 256-key band: most queries are flagged, the early gate and the split-plane form run
    Case("dup-1024-k32", "dup", "fp16", 120_000, 1024, 32, opts=WIDE + (("band_max", 256),), flagged=True),
    # fp32 rows: the filter runs over the fp16 shadow (256-query tiles forced: on so small a corpus the library picks 128)
    Case("shadow-f32-1024-k32", "gauss", "fp32", 60_000, 1024, 32, opts=WIDE + (("mfma_tile", 256),)),
]


def _torch():
    import torch

    return torch


@functools.lru_cache(maxsize=2)
def _corpus(kind: str, rows: int, dtype: str):
    """-> (the values the kernels multiply as float32, device tensor, queries [1024, 1536])"""
    torch = _torch()
    dim = 1536
    if kind == "gauss":
        v, _ = make_corpus(rows, dim, 9100)
        q = make_queries(1024, dim, 9101)
    else:
        v, q, _, _ = make_clustered_corpus(rows, dim, 9102, cluster_rows=100 if kind == "clustered" else 1500, n_queries=1024)
    if dtype == "fp16":
        v16 = v.astype(np.float16)
        return v16.astype(np.float32), torch.from_numpy(v16).cuda(), q
    return v, torch.from_numpy(v).cuda(), q


def _run(eng, dq, k: int, thr: float, shape: int):
    torch = _torch()
    eng.set_option("mfma_shape", shape)
    out = torch.zeros((dq.shape[0], k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    eng.search_device(dq, k, thr, out_keys=out)
    eng.synchronize()
    return out.cpu().numpy().copy(), eng.get_option("last_mfma_shape"), eng.get_option("last_flagged")


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_shapes_agree_bit_for_bit(case):
    torch = _torch()
    v, dev, q = _corpus(case.corpus, case.rows, case.dtype)
    qs = q[: case.nq]
    dq = torch.from_numpy(np.ascontiguousarray(qs)).cuda()
    eng = _native.Engine(0)
    for name, val in case.opts:
        eng.set_option(name, val)
    eng.set_corpus_tensor(dev, ordinal_base=case.base)
    assert len(_native.plan_ladder(case.rows, case.nq)) - 1 >= 3 or case.rows < 200_000
    kth = float(np.sort(vo.scores_full(v, qs[0]))[::-1][min(3, case.rows - 1)])  # a threshold that leaves a handful of rows for query 0
    for thr in (0.0, kth):
        t32 = float(_native.f32_threshold(thr))
        k16, shape16, fl16 = _run(eng, dq, case.k, t32, 16)
        k32, shape32, fl32 = _run(eng, dq, case.k, t32, 32)
        assert (shape16, shape32) == (16, 32), f"{case.name}: last_mfma_shape {shape16} / {shape32}"
        assert eng.get_option("last_shadow") == (case.dtype == "fp32")
        if case.flagged and thr == 0.0:
            assert fl16 > case.nq // 2 and fl32 > case.nq // 2, f"{case.name}: flagged {fl16} / {fl32}"
        assert np.array_equal(k16, k32), f"{case.name} thr={thr}: {int((k16 != k32).sum())} of {k16.size} keys differ between the shapes"
        ords, scs, cnts = _native.decode_keys(k16)
        for qi in sorted({0, 1, case.nq // 2, case.nq - 1}):
            m = int(cnts[qi])
            got = ords[qi, :m] - case.base
            vo.check_topk_parity(vo.scores_full(v, qs[qi]), got, scs[qi, :m], case.k, thr, referee=vo.f64_referee(v, qs[qi]))
    eng.close()


def test_option_validation_and_dispatch():
    torch = _torch()
    v, dev, q = _corpus("gauss", 200_003, "fp16")
    eng = _native.Engine(0)
    assert eng.get_option("mfma_shape") == 16 and eng.get_option("last_mfma_shape") == 0
    for bad in (0, 8, 31, 64):
        with pytest.raises(Exception, match="mfma_shape"):
            eng.set_option("mfma_shape", bad)
    assert eng.get_option("mfma_shape") == 16
    eng.set_option("direct_group_max_nq", 0)
    eng.set_corpus_tensor(dev)
    dq = torch.from_numpy(np.ascontiguousarray(q[:1024])).cuda()
    # the 128-query tile and the direct-query-operand variant stay on 32x32x16 whatever the option says
    eng.set_option("mfma_tile", 128)
    _, shape, _ = _run(eng, dq[:128], 32, 0.0, 16)
    assert shape == 32
    eng.set_option("mfma_tile", 0)
    eng.set_option("mfma_bdirect", 1)
    _, shape, _ = _run(eng, dq, 32, 0.0, 16)
    assert shape == 32
    eng.set_option("mfma_bdirect", 0)
    _, shape, _ = _run(eng, dq, 32, 0.0, 16)
    assert shape == 16
    eng.close()
