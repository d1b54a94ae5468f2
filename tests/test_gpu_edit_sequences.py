"""GPU suite: lookups after row edits on every route that reads a per-corpus cache -- the case table of tests/edit_sequence_cases.py.

Every sequence starts from WARM caches (a forced wide-tile batch: `norm_rows` == rows, `last_shadow` where the kind has a shadow) and after every
step every leg of the kind asserts, in this order:
  1. `norm_rows` right after the edit is what DESIGN 3.12 - 3.13 says (the table's model), and equals the row count after the next wide batch;
  2. the leg's getters: a leg that ran on another route fails;
  3. ordinals identical to the numpy oracle over the model and scores within SCORE_TOL; a differing list goes to the float64 referee
     (`check_topk_parity`), which -- the CPU twin shows more than 1e-4 at rank k of every non-planted query -- can forgive nothing there;
  4. where the leg says `stream_scores`: the batch equals the single streaming lookups bit for bit;
  5. last: equality with a fresh index over the model.
A failure names the case, the step and the leg.  Then: the adversarial cases of the cached maxima (both of them, and non-finite rows), a
scatter of more than two staging chunks, and the class-side caches (the subset cache, a captured graph, the row -> message map)."""

import numpy as np
import pytest

from oracle import messages_oracle as mo
from oracle import vectorbase_oracle as vo
from tests import edit_sequence_cases as ec
from tests.fakes import NullModel
from tests.synth import make_corpus, make_queries
from tests.test_gpu_parity import SCORE_TOL, new_vb
from typeagent_py_amd import TextEmbeddingIndexSettings, VectorBase, _native

pytestmark = pytest.mark.gpu


def _pairs(res):
    return [(r.item, r.score) for r in res]


def _index(kind, keep_host_copy=True, raw=None, msgs=None):
    """ROWS - 1 rows, then the last: the second append doubles the device buffer, so that later edits happen in place"""
    if raw is None:
        raw, msgs, _, _, _ = ec.base(kind)
    vb = VectorBase(TextEmbeddingIndexSettings(NullModel()), corpus_dtype=kind.dtype, keep_host_copy=keep_host_copy)
    vb.add_embeddings(None, raw[:-1].copy())
    assert vb.engine.rows == len(raw) - 1
    vb.add_embeddings(None, raw[-1:].copy())
    assert vb.engine.rows == len(raw) and vb.engine.corpus.shape[0] == 2 * (len(raw) - 1)
    if msgs is not None:
        vb.set_row_messages(msgs)
    return vb


def _handles(vb, cp):
    made = {}
    for s in cp.scopes:
        if id(s) not in made:
            made[id(s)] = vb.row_mask(s)
    return {"mask": vb.row_mask(cp.mask), "scopes": [made[id(s)] for s in cp.scopes]}


def run_leg(vb, kind, leg, qs, handles=None):
    """-> (one list of (item, score) per query, the leg's getters after the call)"""
    eng = vb.engine
    thr = ec.min_score_of(leg, kind)
    opts = ec.leg_opts(leg)
    saved = [(n, eng.get_option(n)) for n, _ in opts]
    profiled = any(g == "topk_launches" for g, _ in leg.expect)
    for n, val in opts:
        eng.set_option(n, val)
    try:
        if profiled:
            eng.profile_enable(True)
            eng.profile_reset()
        if leg.call == "single":
            out = [_pairs(vb.fuzzy_lookup_embedding(q, leg.k, thr)) for q in qs]
        elif leg.call == "batch":
            out = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, leg.k, thr)]
        elif leg.call == "masked":
            out = [_pairs(r) for r in vb.fuzzy_lookup_embeddings_masked(qs, handles["mask"], leg.k, thr)]
        elif leg.call == "scoped":
            out = [_pairs(r) for r in vb.fuzzy_lookup_embeddings_scoped(qs, handles["scopes"], leg.k, thr)]
        elif leg.call == "messages":
            out = [_pairs(vb.lookup_messages_by_embedding(q, leg.k, thr)) for q in qs]
        else:
            out = [_pairs(r) for r in vb.lookup_messages_by_embeddings_scoped(qs, handles["scopes"], leg.k, thr)]
        state = {g: (eng.profile_read(_native.KERNEL_TOPK)[1] if g == "topk_launches" else eng.get_option(g)) for g, _ in leg.expect}
    finally:
        if profiled:
            eng.profile_enable(False)
        for n, val in saved:
            eng.set_option(n, val)
    return out, state


def check_hits(where, ref, sub, q, hits, k, thr, cand=None, planted=False):
    """`hits` against the oracle's float32 scores `ref` of the candidate rows `sub` (the corpus rows `cand`, or all)"""
    items, scores = [i for i, _ in hits], [s for _, s in hits]
    t32 = _native.f32_threshold(thr)
    pos, sc = vo._select_desc(ref, k, t32)
    want = (pos if cand is None else cand[pos]).tolist()
    try:
        if items == want:
            np.testing.assert_allclose(scores, sc, atol=SCORE_TOL, rtol=0)
            return
        if not planted:
            assert sorted(items) == sorted(want), f"rows {sorted(set(items) - set(want))[:6]} for {sorted(set(want) - set(items))[:6]}"
        vo.check_topk_parity(ref, items, scores, k, float(t32), candidate_ordinals=cand, referee=vo.f64_referee(sub, q))
    except AssertionError as err:
        raise AssertionError(f"{where}: {err}") from None


def check_leg(what, kind, leg, cp, qs, v, msgs, out, state, singles):
    where = f"{what} leg {leg.name}"
    for g, allowed in leg.getters(kind):
        assert state[g] in allowed, f"{where}: {g} = {state[g]}, expected {list(allowed)[:6]} (all getters: {state})"
    thr = ec.min_score_of(leg, kind)
    assert len(out) == len(qs), where
    if leg.call in ("single", "batch"):
        ref = vo.cosine_to_score(v @ qs.T)
        for qi, q in enumerate(qs):
            check_hits(f"{where} query {qi}", np.ascontiguousarray(ref[:, qi]), v, q, out[qi], leg.k, thr, planted=leg.planted and qi == len(qs) - 1)
    elif leg.call == "masked":
        flat = np.flatnonzero(cp.mask)
        sub = v[flat]
        ref = vo.cosine_to_score(sub @ qs.T)
        for qi, q in enumerate(qs):
            check_hits(f"{where} query {qi}", np.ascontiguousarray(ref[:, qi]), sub, q, out[qi], leg.k, thr, cand=flat)
    elif leg.call == "scoped":
        for qi, q in enumerate(qs):
            flat = np.flatnonzero(cp.scopes[qi])
            sub = v[flat]
            check_hits(f"{where} query {qi}", vo.cosine_to_score(sub @ q), sub, q, out[qi], leg.k, thr, cand=flat)
    else:
        for qi, q in enumerate(qs):
            if leg.call == "messages":
                want = mo.sqlite_lookup_by_embedding(lambda e, k, t: vo.lookup(v, e, k, t), q, msgs, leg.k, thr, None)
            else:
                flat = np.flatnonzero(cp.scopes[qi])
                hits = vo.lookup_in_subset(v, q, flat, leg.k, thr)
                want = mo.memory_messages_from_hits([(p, s) for p, s in hits if msgs[p] >= 0], msgs)[: leg.k]
            # the same messages (the rows are determinate: more than 1e-4 at rank k), every message with the oracle's score, and rank by rank the
            # oracle's score: two messages may change places only where their scores are within the tolerance of each other
            best = dict(want)
            assert sorted(m for m, _ in out[qi]) == sorted(best), f"{where} query {qi}: messages {[m for m, _ in out[qi]][:8]}, the oracle's {[m for m, _ in want][:8]}"
            np.testing.assert_allclose([s for _, s in out[qi]], [best[m] for m, _ in out[qi]], atol=SCORE_TOL, rtol=0, err_msg=f"{where} query {qi}")
            np.testing.assert_allclose([s for _, s in out[qi]], [s for _, s in want], atol=SCORE_TOL, rtol=0, err_msg=f"{where} query {qi}")
    if leg.call in ("single", "batch", "masked", "scoped") and leg.name not in ("large-k", "sort-all"):
        for qi, (aim, row) in enumerate(cp.aimed[: len(qs) - int(leg.planted)]):
            if row >= 0:
                assert out[qi] and out[qi][0][0] == row, f"{where} query {qi}: aimed at the {aim} row {row}, found {out[qi][:1]}"
    if leg.stream_scores and singles is not None:
        for qi in range(len(qs) - int(leg.planted)):  # (the cluster's query is re-run on an exact tile with its own summation order: the referee's)
            assert out[qi] == singles[qi], f"{where} query {qi}: the batch differs from the single lookup: {out[qi][:3]} / {singles[qi][:3]}"


def singles_of(vb, kind, leg, cp, qs, anchor):
    """the single lookups a `stream_scores` leg must equal: the streaming kernel's over the corpus, or over the leg's row list"""
    thr = ec.min_score_of(leg, kind)
    if not leg.stream_scores or leg.call in ("single", "messages", "messages_scoped"):
        return None
    if leg.call == "batch":
        if leg.name in ("large-k", "sort-all"):
            return [_pairs(vb.fuzzy_lookup_embedding(q, leg.k, thr)) for q in qs]
        out = [a[: leg.k] for a in anchor[: len(qs)]]  # (the best k of the anchor's 32, whose selection is exact)
        if leg.planted:
            out[-1] = _pairs(vb.fuzzy_lookup_embedding(qs[-1], leg.k, thr))
        return out
    if leg.call == "masked":
        flat = np.flatnonzero(cp.mask)
        return [_pairs(vb.fuzzy_lookup_embedding_in_subset(q, flat, leg.k, thr)) for q in qs]
    return [_pairs(vb.fuzzy_lookup_embedding_in_subset(q, np.flatnonzero(cp.scopes[qi]), leg.k, thr)) for qi, q in enumerate(qs)]


def run_checkpoint(what, vb, kind, e, cp):
    model = e.model
    v = ec.seen(kind, model.raw)
    eng = vb.engine
    handles = _handles(vb, cp)
    results = {}
    anchor = None
    for leg in ec.legs_of(kind):
        qs = ec.leg_queries(leg, cp)
        out, state = run_leg(vb, kind, leg, qs, handles)
        if leg.name == "single":
            anchor = out
            assert eng.get_option("norm_rows") == e.norm_rows, f"{what}: the streaming lookups changed norm_rows"  # they read only the corpus
        check_leg(what, kind, leg, cp, qs, v, model.msgs, out, state, singles_of(vb, kind, leg, cp, qs, anchor))
        if leg.extends_norms:
            assert eng.get_option("norm_rows") == len(model), f"{what} leg {leg.name}: norm_rows {eng.get_option('norm_rows')} of {len(model)} rows"
        results[leg.name] = out
    # (the masked tile's options switch the fp16 shadow off and on again: the checkpoint ends as it began, with every row covered)
    run_leg(vb, kind, ec.WARM, cp.queries)
    assert eng.get_option("norm_rows") == len(model) and eng.get_option("last_shadow") == kind.shadow, what
    fresh = new_vb(model.raw, kind.dtype)
    fresh.set_row_messages(model.msgs)
    fresh_handles = _handles(fresh, cp)
    for leg in ec.legs_of(kind):
        out, _ = run_leg(fresh, kind, leg, ec.leg_queries(leg, cp), fresh_handles)
        assert out == results[leg.name], f"{what} leg {leg.name}: differs from a fresh index over the model"
    return handles


@pytest.mark.parametrize("case", ec.CASES, ids=[c.id for c in ec.CASES])
def test_lookups_after_every_step_of_a_sequence(case):
    kind, seq = case.kind, case.sequence
    vb = _index(kind, seq.keep_host_copy)
    eng = vb.engine
    eng.set_option("compact_pass_rows", case.pass_rows)
    pool = ec.base(kind)[4]
    run_leg(vb, kind, ec.WARM, pool[: ec.NQ])
    assert eng.get_option("norm_rows") == ec.ROWS and eng.get_option("last_tier") == 4 and eng.get_option("last_shadow") == kind.shadow, f"{case.id}: not warm"
    old = vb.row_mask(np.arange(ec.ROWS) % 2 == 0)
    for i, (e, cp) in enumerate(ec.checkpoints(kind, seq.name)):
        what = f"{case.id} step {i} ({e.step.op} {e.step.where})"
        tensor = eng.corpus
        ec.apply_edit(vb, e)
        eng = vb.engine
        assert eng.rows == len(e.model) == len(vb), what
        assert eng.corpus is tensor and eng.corpus.shape[0] == e.model.cap, f"{what}: the edit did not happen in place"
        assert eng.get_option("norm_rows") == e.norm_rows, f"{what}: norm_rows {eng.get_option('norm_rows')} right after the edit, expected {e.norm_rows}"
        if not seq.keep_host_copy:
            assert vb._device_only is eng.corpus and vb._host.shape[0] == 0, f"{what}: a device-only corpus was copied to the host"
        if e.call in ("insert_rows", "remove_rows"):
            with pytest.raises(ValueError):
                vb.fuzzy_lookup_embedding_masked(pool[0], old, 5, 0.0)
        elif e.call == "set_rows":
            assert len(vb.fuzzy_lookup_embedding_masked(pool[0], old, 5, 0.0)) == 5  # the handle stays valid
        if cp is not None:
            old = run_checkpoint(what, vb, kind, e, cp)["mask"]
        else:
            old = vb.row_mask(np.arange(len(vb)) % 2 == 0)
    if seq.keep_host_copy:
        np.testing.assert_array_equal(np.asarray(vb.serialize()), e.model.raw)


# ---- the cached maxima, adversarially ------------------------------------------------------------------------------------------------------------
N_ADV, D_ADV = ec.ROWS, 128
F32 = ec.KIND["f32-d128"]


def _wide(vb, qs, k, opts=ec.WIDE, flagged=None, tier=4):
    """a forced wide-tile batch (or, with `opts` and `tier`, another forced route) -> its lists; the getters are asserted"""
    eng = vb.engine
    saved = [(n, eng.get_option(n)) for n, _ in opts]
    for n, val in opts:
        eng.set_option(n, val)
    try:
        out = [_pairs(r) for r in vb.fuzzy_lookup_embeddings(qs, k, 0.0)]
        state = {g: eng.get_option(g) for g in ("last_tier", "last_shadow", "last_flagged", "norm_rows")}
    finally:
        for n, val in saved:
            eng.set_option(n, val)
    assert state["last_tier"] == tier and state["norm_rows"] == len(vb), state
    if flagged is not None:
        assert state["last_flagged"] in flagged, state
    return out, state


def _exact_corpus(n, d, seed):
    """rows whose values are all exact in fp16 (the cached rounding-error norm of their shadow is 0), roughly unit length"""
    rng = np.random.default_rng(seed)
    return (rng.integers(-256, 257, size=(n, d)).astype(np.float32) / 2048.0).astype(np.float32)


def _planted(q, count, rng):
    """tests/test_gpu_routes.py's near-duplicates: rows within fp16 resolution of one another around a direction near the query"""
    d = len(q)
    base = q + 0.3 * rng.standard_normal(d).astype(np.float32) / np.sqrt(d)
    base /= np.linalg.norm(base)
    w = base[None, :] + 2e-4 * rng.standard_normal((count, d)).astype(np.float32) / np.sqrt(d)
    return (w / np.linalg.norm(w, axis=1, keepdims=True)).astype(np.float32)


PLANTED = (1, 3, 5)  # the queries that sit on near-duplicates


@pytest.mark.parametrize("how", ["set_rows", "insert_rows"])
@pytest.mark.parametrize("k", [8, 32])
def test_the_rounding_error_maximum_follows_new_rows(how, k):
    """stats[1]: a corpus exact in fp16 caches a rounding-error norm E of 0.  Then 300 near-duplicates per planted query arrive: unit rows
    2e-4 / sqrt(d) apart per element, about 4e-5 of score end to end and 1e-7 from one to the next, whose fp16 copies are off by about
    1e-5 of score each -- the filter's fp16 order among them says nothing about the fp32 order, only the error bound does.  The bound of a
    query is 0.5 * (|q - q16| R + E |q| + summation slack) (query_prepare_kernel), and the query term alone (7e-5 for a unit query at this
    width) would hide a stale E.  So the planted queries are themselves exact in fp16: their query term is 0, and with a stale E = 0 the band
    is the slack alone, about 3e-6 of score -- true top-k rows fall outside it and the answer is the filter's.  With E folded the band is
    about 2e-4 and holds the whole group.  (`set_rows` keeps the caches, so the scatter kernel's fold is what is tested; `insert_rows` below
    norm_rows rebuilds them.  With the fold taken out of a scratch build, both `set_rows` cases fail by a wrong ordinal.)"""
    route = "wide"
    v = _exact_corpus(N_ADV, D_ADV, 51_000)
    assert np.array_equal(v.astype(np.float16).astype(np.float32), v)
    nq, opts, tier = ec.NQ, ec.WIDE, 4
    qs = make_queries(nq, D_ADV, 51_001)
    rng = np.random.default_rng(51_002)
    for qi in PLANTED:
        qs[qi] = qs[qi].astype(np.float16).astype(np.float32)  # exact in fp16 (and unit length to 1e-4)
    vb = _index(F32, raw=v)
    _wide(vb, qs, k, opts, tier=tier)
    assert vb.engine.get_option("last_shadow") == 1
    new = np.concatenate([_planted(qs[qi], 300, rng) for qi in PLANTED])
    assert not np.array_equal(new.astype(np.float16).astype(np.float32), new)
    if how == "set_rows":
        which = rng.choice(N_ADV, size=len(new), replace=False)
        assert vb.set_rows(which, new) == len(new)
        model = v.copy()
        model[which] = new
        assert vb.engine.get_option("norm_rows") == N_ADV  # the caches are kept: the scatter kernel has to fold the new rows' error norms
    else:
        at = np.full(len(new), N_ADV)  # half behind the last row, half in the upper half of the corpus: the caches are rebuilt
        at[: len(new) // 2] = rng.integers(N_ADV // 2, N_ADV, size=len(new) // 2)
        assert vb.insert_rows(at, new) == len(new)
        model = np.insert(v, at, new, axis=0)
        assert vb.engine.get_option("norm_rows") == 0
    got, state = _wide(vb, qs, k, opts, tier=tier)
    assert state["last_shadow"] == 1
    for qi, q in enumerate(qs):
        where = f"stats[1] {route} {how} k {k} query {qi}"
        check_hits(where, vo.scores_full(model, q), model, q, got[qi], k, 0.0, planted=True)  # (the referee decides every difference)
        assert got[qi] == _pairs(vb.fuzzy_lookup_embedding(q, k, 0.0)), where
    fresh = new_vb(model, "fp32")
    assert got == _wide(fresh, qs, k, opts, tier=tier)[0]


@pytest.mark.parametrize("kind", [F32, ec.KIND["f16-d128"], ec.KIND["f16-d100"]], ids=lambda k: k.name)
@pytest.mark.parametrize("k", [8, 32])
def test_the_norm_maximum_follows_new_rows_and_stays_an_upper_bound(kind, k):
    """stats[0]: a new row four times as long and one a hundredth as long; and the reverse, a row a thousand times as long overwritten by a
    unit row: the stale maximum is only an upper bound, every answer stays exact (`last_flagged` may grow)."""
    raw, _, _, _, pool = ec.base(kind)
    qs = pool[: ec.NQ].copy()
    extra, _ = make_corpus(4, kind.dim, 52_000)
    for how in ("set_rows", "insert_rows"):
        start = raw.copy()
        start[777] = 1000.0 * raw[777]
        vb = _index(kind, raw=start)
        _wide(vb, qs, k)
        rows = np.stack([4.0 * extra[0], 0.01 * extra[1], extra[2]])
        qs[7], qs[9], qs[11] = extra[0], extra[1], extra[2]
        if how == "set_rows":
            which = np.array([5000, ec.CHUNK, 777])  # the last: the long row goes
            vb.set_rows(which, rows)
            model = start.copy()
            model[which] = rows
            assert vb.engine.get_option("norm_rows") == ec.ROWS
        else:
            vb.set_rows([777], rows[2:])
            vb.insert_rows([5000, ec.ROWS], rows[:2])
            model = start.copy()
            model[777] = rows[2]
            model = np.insert(model, [5000, ec.ROWS], rows[:2], axis=0)
        v = ec.seen(kind, model)
        got, state = _wide(vb, qs, k, flagged=range(0, ec.NQ + 1))
        assert state["last_shadow"] == kind.shadow
        for qi, q in enumerate(qs):
            where = f"stats[0] {kind.name} {how} k {k} query {qi}"
            check_hits(where, vo.scores_full(v, q), v, q, got[qi], k, 0.0, planted=True)
            assert got[qi] == _pairs(vb.fuzzy_lookup_embedding(q, k, 0.0)), where
        assert got[7][0][0] == 5000  # the long row leads its own query, as it does on the streaming kernel


@pytest.mark.parametrize("how", ["set_rows", "insert_rows"])
def test_non_finite_rows_arrive_by_an_edit(how):
    """A NaN-bearing and an inf-bearing row: the answers equal the single streaming lookups and the same matrix freshly uploaded, bit for bit,
    and the oracle's the way tests/test_gpu_parity.py asks it about such rows: the NaN row is never returned, the inf row scores 1 or 0."""
    kind = F32
    raw, _, _, _, pool = ec.base(kind)
    qs = pool[: ec.NQ]
    vb = _index(kind)
    _wide(vb, qs, 8)
    bad = raw[:2].copy()
    bad[0, 5] = np.nan
    bad[1, 9] = np.inf
    if how == "set_rows":
        vb.set_rows([100, ec.CHUNK], bad)
        model = raw.copy()
        model[[100, ec.CHUNK]] = bad
        assert vb.engine.get_option("norm_rows") == ec.ROWS
    else:
        vb.insert_rows([100, ec.CHUNK], bad)
        model = np.insert(raw, [100, ec.CHUNK], bad, axis=0)
    nan_row = int(np.flatnonzero(np.isnan(model).any(axis=1))[0])
    inf_row = int(np.flatnonzero(np.isinf(model).any(axis=1))[0])
    assert nan_row == 100 and inf_row == ec.CHUNK + (how == "insert_rows")
    fresh = new_vb(model, "fp32")
    led = 0
    for k in (8, 32):
        got, _ = _wide(vb, qs, k, flagged=range(0, ec.NQ + 1))
        assert got == _wide(fresh, qs, k, flagged=range(0, ec.NQ + 1))[0], f"non-finite {how} k {k}: differs from a fresh upload"
        for qi, q in enumerate(qs):
            where = f"non-finite {how} k {k} query {qi}"
            assert got[qi] == _pairs(vb.fuzzy_lookup_embedding(q, k, 0.0)), f"{where}: differs from the single lookup"
            items, scores = [i for i, _ in got[qi]], [s for _, s in got[qi]]
            assert nan_row not in items, f"{where}: the NaN row was returned"
            with np.errstate(invalid="ignore", over="ignore"):
                sc = vo.scores_full(model, q)
                vo.check_topk_parity(sc, items, scores, k, 0.0)
            if q[9] > 0:  # +inf times a positive weight: the row's score is clipped to 1 and leads
                assert got[qi][0] == (inf_row, 1.0), where
                led += 1
            else:
                assert inf_row not in items, where
    assert led >= 20  # (both signs of the weight occur among the queries)


# ---- more than two staging chunks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_a_scatter_of_three_staging_chunks_places_every_row(dtype):
    """6000 x 2048: 2048 rows per 16 MiB chunk, so 4200 rows are three chunks and the wait for a staging slot is taken.  Each new row is a
    function of its destination: a wrong offset into the positions on chunk 2 or 3 misplaces rows."""
    n, d, m = 6000, 2048, 4200
    kind = ec.Kind(f"{dtype}-d{d}", dtype, d)
    v, _ = make_corpus(n, d, 53_000)
    vb = _index(kind, raw=v)
    qs = make_queries(ec.NQ, d, 53_001)
    _wide(vb, qs, 8)
    rng = np.random.default_rng(53_002)

    def rows_for(dest):  # the destination is written into the row
        rows = make_corpus(len(dest), d, 53_003)[0]
        rows[:, 0] = (dest % 64) / 64.0
        rows[:, 1] = (dest // 64) / 128.0
        return (rows / np.linalg.norm(rows, axis=1, keepdims=True)).astype(np.float32)

    which = rng.permutation(n)[:m]
    new = rows_for(which)
    assert vb.set_rows(which, new) == m
    model = v.copy()
    model[which] = new

    def check(model, aim):
        fresh = new_vb(model, dtype)
        got = vb.engine.corpus[: len(model)].cpu().numpy()
        want = fresh.engine.corpus[: len(model)].cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), "the device corpus differs from a fresh upload"
        seen = ec.seen(kind, model)
        q2 = qs.copy()
        q2[: len(aim)] = seen[aim] / np.linalg.norm(seen[aim], axis=1, keepdims=True)
        out, _ = _wide(vb, q2, 8)
        for qi, q in enumerate(q2):
            check_hits(f"three chunks {dtype} query {qi}", vo.scores_full(seen, q), seen, q, out[qi], 8, 0.0, planted=True)
        for qi, r in enumerate(aim):
            assert out[qi][0][0] == int(r)

    check(model, np.concatenate([which[2048:2052], which[4096:4100], which[-2:]]))  # rows of the second and of the third chunk
    at = np.sort(rng.integers(0, n + 1, size=m))
    pos = ec.positions_of(at, n, m)
    new = rows_for(pos)
    assert vb.insert_rows(at, new) == m
    model = np.insert(model, at, new, axis=0)
    assert np.array_equal(model[pos], new)
    check(model, np.concatenate([pos[2048:2052], pos[4096:4100], pos[-2:]]))


# ---- the class-side caches -----------------------------------------------------------------------------------------------------------------------
def test_the_subset_cache_a_captured_graph_and_the_message_map_follow_edits():
    n, d = 3000, 64
    v, q = make_corpus(n, d, 54_000)
    extra, _ = make_corpus(8, d, 54_001)
    rng = np.random.default_rng(54_002)
    msgs = np.sort(rng.integers(0, n // 3, size=n)).astype(np.int64)
    vb = new_vb(v)
    vb.set_row_messages(msgs)
    model = v.copy()

    def same(res, want, what):
        assert [i for i, _ in _pairs(res)] == [i for i, _ in want], what
        np.testing.assert_allclose([s for _, s in _pairs(res)], [s for _, s in want], atol=SCORE_TOL, rtol=0, err_msg=what)

    # the subset cache: the same list object before and after set_rows
    subset = rng.choice(n, size=400, replace=False).tolist()
    same(vb.fuzzy_lookup_embedding_in_subset(q, subset, 10, 0.0), vo.lookup_in_subset(model, q, subset, 10, 0.0), "subset before")
    cached = vb._subset_cache[4]
    assert vb._subset_cache[0] is subset
    target = subset[17]
    assert vb.set_rows([target], q) == 1
    model[target] = q
    got = vb.fuzzy_lookup_embedding_in_subset(q, subset, 10, 0.0)
    assert vb._subset_cache[4] is cached, "set_rows dropped the cached device row list"
    same(got, vo.lookup_in_subset(model, q, subset, 10, 0.0), "subset after set_rows")
    assert got[0].item == target
    assert vb.insert_rows([0, target], extra[:2]) == 2
    model = np.insert(model, [0, target], extra[:2], axis=0)
    msgs = np.insert(msgs, [0, target], [-1, -1])
    assert vb._subset_cache is None
    subset = [s + 2 for s in subset]
    got = vb.fuzzy_lookup_embedding_in_subset(q, subset, 10, 0.0)
    same(got, vo.lookup_in_subset(model, q, subset, 10, 0.0), "subset after insert_rows")
    assert vb.remove_rows([0, 5]) == 2 and vb._subset_cache is None
    model, msgs = np.delete(model, [0, 5], axis=0), np.delete(msgs, [0, 5])
    subset = [s - 2 for s in subset if s > 5]
    same(vb.fuzzy_lookup_embedding_in_subset(q, subset, 10, 0.0), vo.lookup_in_subset(model, q, subset, 10, 0.0), "subset after remove_rows")

    # a captured graph replays after set_rows and sees the new contents; an in-place removal and an append are seen too
    eng = vb.engine
    eng.set_option("graph_max_bytes", 256 << 20)
    q2 = make_queries(1, d, 54_003)[0]
    for _ in range(4):
        res = vb.fuzzy_lookup_embedding(q2, 10, 0.0)
        if eng.get_option("last_graph") == 1:
            break
    assert eng.get_option("last_graph") == 1
    same(res, vo.lookup(model, q2, 10, 0.0), "graph before")
    top = res[0].item
    vb.set_rows([top], -q2)
    model[top] = -q2
    res = vb.fuzzy_lookup_embedding(q2, 10, 0.0)
    assert vb.engine.get_option("last_graph") == 1, "set_rows keeps the corpus where it was: the captured graph replays"
    same(res, vo.lookup(model, q2, 10, 0.0), "graph after set_rows")
    assert res[0].item != top
    tensor = eng.corpus
    assert vb.remove_rows([res[0].item]) == 1 and vb.engine.corpus is tensor
    model, msgs = np.delete(model, [res[0].item], axis=0), np.delete(msgs, [res[0].item])
    for _ in range(3):
        same(vb.fuzzy_lookup_embedding(q2, 10, 0.0), vo.lookup(model, q2, 10, 0.0), "graph after remove_rows")
    vb.add_embeddings(None, q2[None])
    model, msgs = np.concatenate([model, q2[None]]), np.concatenate([msgs, [7]])
    vb.set_row_messages(msgs)
    for _ in range(3):
        res = vb.fuzzy_lookup_embedding(q2, 10, 0.0)
        same(res, vo.lookup(model, q2, 10, 0.0), "graph after an append")
    assert res[0].item == len(model) - 1
    eng.set_option("graph_max_bytes", 0)

    # the row -> message map after each edit kind
    def messages(what):
        scope_msgs = [np.unique(msgs[msgs >= 0])[i::3] for i in range(3)]
        scopes = [vb.message_mask(s) for s in scope_msgs]
        qs = np.stack([q, q2, model[50]])
        got = vb.lookup_messages_by_embeddings_scoped(qs, scopes, 10, 0.0)
        assert vb.engine.get_option("masked_route") == 4
        for i in range(3):
            allowed = np.isin(msgs, scope_msgs[i]) & (msgs >= 0)
            np.testing.assert_array_equal(scopes[i].flat(), np.flatnonzero(allowed), err_msg=what)
            hits = vo.lookup_in_subset(model, qs[i], np.flatnonzero(allowed), 10, 0.0)
            want = mo.memory_messages_from_hits(hits, msgs)[:10]
            assert [m for m, _ in _pairs(got[i])] == [m for m, _ in want], (what, i)
            np.testing.assert_allclose([s for _, s in _pairs(got[i])], [s for _, s in want], atol=SCORE_TOL, rtol=0)

    messages("after the edits above")
    vb.set_rows([50, 60], extra[2:4])
    model[[50, 60]] = extra[2:4]
    messages("after set_rows")
    vb.insert_rows([10, 2000], extra[4:6], row_messages=[3, 900])
    model, msgs = np.insert(model, [10, 2000], extra[4:6], axis=0), np.insert(msgs, [10, 2000], [3, 900])
    messages("after insert_rows")
    gone = np.arange(40, 90)
    vb.remove_rows(gone)
    model, msgs = np.delete(model, gone, axis=0), np.delete(msgs, gone)
    messages("after remove_rows")
