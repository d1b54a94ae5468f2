"""The case table of tests/test_gpu_edit_sequences.py and of its CPU twin tests/test_edit_sequence_cases_host.py: lookups after row edits on
every route that reads a per-corpus cache -- the fp16 shadow of an fp32 corpus, the zero-padded copy of an odd-width fp16 corpus, the row-norm
maxima ("norm_rows" rows of them), the subset cache, the captured graphs, the device row -> message map.

A case is a corpus KIND (the smallest shapes that have each cache, CHUNK + 1 rows: one mask chunk and one row), a SEQUENCE of edit steps, each
applied to the index and to a numpy MODEL (np.insert / np.delete / index assignment; the model also says what `norm_rows` and the capacity of
the device buffer must be after the step), and the route LEGS checked after every step.  The queries of a checkpoint are
chosen so that a stale cache changes the answer: the new rows themselves, rows that moved (just behind the first edit position, and at the
very end), rows in front of it, and the old contents of overwritten or removed rows; the rest come from a pool.  Every query is kept only if
the float32 scores of the model leave more than MARGIN between rank k and rank k + 1 (and, for a query aimed at a row, between that row and
rank 2) under every (k, mask) a leg uses it with; the CPU twin asserts GAP on the float64 scores, so that no comparison on the device can be
forgiven as a tie.  One cluster of CLUSTER near-duplicates of one query serves the flagged-query leg, which goes through the float64 referee.

A plain module (numpy only; no test, no fixture): both test files import it.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

from tests import remove_rows_cases as rc
from tests.synth import make_corpus, make_queries
from tests.test_gpu_routes import FLAG, SHADOW, TILE, WIDE  # the option tuples that force a route (importing that module needs no GPU)

CHUNK = rc.CHUNK
ROWS = CHUNK + 1
CAPACITY = 2 * (ROWS - 1)  # the index is filled in two appends (ROWS - 1 rows, then one): the second doubles the device buffer, later edits fit in place
PASSES = (0, 128)  # "compact_pass_rows": the library's default, and passes of two tiles (an in-place insert or removal takes over a hundred)
CLUSTER = 300  # near-duplicates of the cluster query: more than band_max = 256
GAP = 1e-4  # what the CPU twin asserts on float64 scores
MARGIN = 2e-4  # what the selection asks of float32 scores
NQ = 66  # queries per checkpoint: one more than the fewest the wide tile takes on fp16 corpora


@dataclass(frozen=True)
class Kind:
    name: str
    dtype: str
    dim: int

    @property
    def f32(self) -> bool:
        return self.dtype == "fp32"

    @property
    def shadow(self) -> int:
        """what `last_shadow` reports after a wide batch: the fp16 shadow of fp32 rows, the padded copy of an odd width"""
        return int(self.f32 or self.dim % 64 != 0)

    @property
    def tile(self) -> bool:
        """the 32/64-query tile serves rows of whole 64-byte steps (skinny_supported)"""
        return (self.dim * (4 if self.f32 else 2)) % 64 == 0

    @property
    def seed(self) -> int:
        return 41_000 + 1000 * self.dim + int(self.f32)


KINDS = (Kind("f32-d128", "fp32", 128), Kind("f16-d100", "fp16", 100), Kind("f16-d72", "fp16", 72), Kind("f16-d128", "fp16", 128))
KIND = {k.name: k for k in KINDS}


def seen(kind: Kind, x: np.ndarray) -> np.ndarray:
    """the values the kernels multiply: fp16 corpora hold the rounded rows"""
    x = np.asarray(x, dtype=np.float32)
    return x if kind.f32 else x.astype(np.float16).astype(np.float32)


# ---- route legs ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Leg:
    name: str
    call: str  # "single", "batch", "masked", "scoped", "messages", "messages_scoped"
    nq: int
    k: int
    opts: tuple = ()
    expect: tuple = ()  # (getter, allowed values)
    stream_scores: bool = True  # the batch equals the single streaming lookups bit for bit
    planted: bool = False  # the last query is the cluster's: through the referee
    needs: str = ""  # "f32", "f16", "tile": the kinds that have the route
    extends_norms: bool = False  # the route ends in search_wide_exact: afterwards norm_rows == rows
    min_score: float = 0.0

    def applies(self, kind: Kind) -> bool:
        return {"": True, "f32": kind.f32, "f16": not kind.f32, "tile": kind.tile}[self.needs]

    def getters(self, kind: Kind) -> tuple:
        """the leg's expectations with the kind's own values filled in"""
        out = []
        for g, allowed in self.expect:
            if allowed == "shadow":
                allowed = (kind.shadow,)
            elif allowed == "skinny":
                from tests import skinny_cases as sc

                allowed = (sc.kernel_id(kind.dim, kind.f32, sc.query_tile(self.nq)),)
            out.append((g, allowed))
        return tuple(out)


def _masked_tile_opts():
    from tests import masked_tile_cases as mt

    return mt.ROUTE_OPTS


def _masked_wide_opts():
    from tests import masked_wide_cases as mw

    return mw.ROUTE_OPTS + WIDE


LEGS = (
    # the anchor: one query at a time on the streaming kernels, which read only the corpus
    Leg("single", "single", NQ, 32, (), (("last_graph", (0,)),)),
    Leg("tile32", "batch", 24, 32, TILE, (("last_tier", (5,)), ("last_shadow", (0,)), ("last_skinny_kernel", "skinny")), stream_scores=False, needs="tile"),
    Leg("tile64", "batch", 40, 8, TILE, (("last_tier", (5,)), ("last_shadow", (0,)), ("last_skinny_kernel", "skinny")), stream_scores=False, needs="tile"),
    Leg("shadow-tile", "batch", 16, 32, SHADOW, (("last_tier", (5,)), ("last_shadow", (1,))), needs="f32", extends_norms=True),
    Leg("wide128", "batch", NQ, 8, WIDE + (("mfma_tile", 128),), (("last_tier", (4,)), ("last_shadow", "shadow"), ("last_mfma_shape", (32,)), ("last_flagged", range(0, NQ + 1))),
        extends_norms=True),
    Leg("wide256", "batch", NQ, 32, WIDE + (("mfma_tile", 256),), (("last_tier", (4,)), ("last_shadow", "shadow"), ("last_mfma_shape", (16, 32)), ("last_flagged", range(0, NQ + 1))),
        extends_norms=True),
    Leg("flagged", "batch", NQ, 8, FLAG, (("last_tier", (4,)), ("last_shadow", "shadow"), ("last_flagged", range(1, NQ + 1))), planted=True, extends_norms=True),
    Leg("masked-gather", "masked", 8, 8, (), (("masked_route", (1,)),)),
    Leg("masked-tile32", "masked", 24, 8, "masked_tile", (("masked_route", (2,)), ("last_tier", (5,)), ("last_shadow", (0,)), ("last_skinny_kernel", "skinny")),
        stream_scores=False, needs="tile"),
    Leg("masked-tile64", "masked", 40, 32, "masked_tile", (("masked_route", (2,)), ("last_tier", (5,)), ("last_shadow", (0,)), ("last_skinny_kernel", "skinny")),
        stream_scores=False, needs="tile"),
    Leg("masked-wide", "masked", NQ, 32, "masked_wide", (("masked_route", (3,)), ("last_tier", (4,)), ("last_shadow", "shadow")), needs="f16", extends_norms=True),
    Leg("scoped", "scoped", 8, 8, (), (("masked_route", (4,)),)),
    Leg("large-k", "batch", 3, 300, (), (("topk_launches", range(1, 1000)),)),
    Leg("sort-all", "batch", 3, 0, (), (("topk_launches", range(1, 1000)),), min_score=-1.0),  # (see min_score_of)
    Leg("messages", "messages", 4, 25, (), ()),
    Leg("messages-scoped", "messages_scoped", 8, 8, (), (("masked_route", (4,)),)),
)
LEG = {leg.name: leg for leg in LEGS}
WARM = LEG["wide128"]  # "warm caches": this batch first


def min_score_of(leg: Leg, kind: Kind) -> float:
    """sort-all returns every survivor: a threshold three standard deviations of a random cosine up, a few dozen rows at every width"""
    return round(0.5 + 1.5 / float(np.sqrt(kind.dim)), 4) if leg.min_score < 0 else leg.min_score


def leg_opts(leg: Leg) -> tuple:
    if leg.opts == "masked_tile":
        return _masked_tile_opts()
    if leg.opts == "masked_wide":
        return _masked_wide_opts()
    return leg.opts


def legs_of(kind: Kind) -> tuple:
    return tuple(leg for leg in LEGS if leg.applies(kind))


# ---- edit steps ------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Step:
    op: str  # "append", "insert", "set", "remove", "clear_add"
    where: str = ""
    lookups: bool = True

    @property
    def kind(self) -> tuple:
        return (self.op, self.where)


STEP_KINDS = (("append", ""), ("insert", "front"), ("insert", "middle"), ("insert", "chunk_edge"), ("insert", "tail"), ("set", "below"), ("set", "above"),
              ("set", "straddle"), ("remove", "before"), ("remove", "across"), ("remove", "after"), ("clear_add", ""))
COLD = Step("append", lookups=False)  # a cold tail: rows behind norm_rows, and no lookup that would warm them
LONG = (Step("remove", "before"), Step("append"), Step("insert", "middle"), Step("set", "below"), Step("remove", "before"))


@dataclass(frozen=True)
class Sequence:
    name: str
    steps: tuple
    keep_host_copy: bool = True

    @property
    def moves_rows(self) -> bool:
        """an in-place insert or removal: worth a second run under short passes"""
        return any(s.op in ("insert", "remove") for s in self.steps)


SEQUENCES = (
    Sequence("insert", (Step("insert", "middle"),)),
    Sequence("insert-front", (Step("insert", "front"),)),
    Sequence("insert-chunk-edge", (Step("insert", "chunk_edge"),)),
    Sequence("remove", (Step("remove", "before"),)),
    Sequence("set", (Step("set", "below"),)),
    Sequence("cold-set-straddle", (COLD, Step("set", "straddle"))),
    Sequence("cold-set-above", (COLD, Step("set", "above"))),
    Sequence("cold-insert-tail", (COLD, Step("insert", "tail"))),
    Sequence("cold-remove-across", (COLD, Step("remove", "across"))),
    Sequence("cold-remove-after", (COLD, Step("remove", "after"))),
    Sequence("clear-add", (Step("clear_add"),)),
    Sequence("long", LONG),
    Sequence("long-device-only", LONG, keep_host_copy=False),
)
SEQUENCE = {s.name: s for s in SEQUENCES}


@dataclass(frozen=True)
class Case:
    kind: Kind
    sequence: Sequence
    pass_rows: int

    @property
    def id(self) -> str:
        return f"{self.kind.name}-{self.sequence.name}-pass{self.pass_rows}"


CASES = tuple(Case(k, s, p) for k in KINDS for s in SEQUENCES for p in PASSES if p == 0 or s.moves_rows)


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Model:
    raw: np.ndarray  # float32 [n, dim]: the rows as they were handed to the index
    msgs: np.ndarray  # int64 [n]: row -> message (-1: none)
    tag: np.ndarray  # int8 [n]: 1 = a row of the cluster
    norm_rows: int  # what option "norm_rows" must report
    cap: int  # rows of the device buffer

    def __len__(self) -> int:
        return len(self.raw)


@dataclass
class Edit:
    """One step, ready to apply: `call` names the method, `args` its arguments; `model` is the state afterwards."""
    step: Step
    call: str
    args: dict
    model: Model
    first: int  # the first row whose ordinal or contents changed
    aimed: list = field(default_factory=list)  # (what, vector, the row of `model` it must find or -1)
    map_again: bool = False  # the caller hands the row -> message map over again (an append does not extend it)
    norm_rows: int = 0  # what option "norm_rows" must report right after the step, before any lookup


@functools.lru_cache(maxsize=4)
def base(kind: Kind):
    """-> (raw rows [ROWS, dim], row -> message, cluster tags, the cluster's query, the pool of fill queries)"""
    raw, _ = make_corpus(ROWS, kind.dim, kind.seed)
    rng = np.random.default_rng(kind.seed + 1)
    c = make_queries(1, kind.dim, kind.seed + 2)[0]
    where = rng.choice(ROWS, size=CLUSTER, replace=False)
    w = c[None, :] + 2e-4 * rng.standard_normal((CLUSTER, kind.dim)).astype(np.float32) / np.sqrt(kind.dim)
    raw[where] = w / np.linalg.norm(w, axis=1, keepdims=True)
    tag = np.zeros(ROWS, dtype=np.int8)
    tag[where] = 1
    msgs = np.sort(rng.integers(0, ROWS // 3, size=ROWS)).astype(np.int64)
    msgs[rng.choice(ROWS, size=50, replace=False)] = -1
    pool = make_queries(420, kind.dim, kind.seed + 3)
    for a in (raw, tag, msgs, c, pool):
        a.setflags(write=False)
    return raw, msgs, tag, c, pool


def start(kind: Kind) -> Model:
    """the warm index: every row covered by the caches"""
    raw, msgs, tag, _, _ = base(kind)
    return Model(raw.copy(), msgs.copy(), tag.copy(), ROWS, CAPACITY)


def _unit(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return (x / np.linalg.norm(x, axis=-1, keepdims=True)).astype(np.float32)


def _plain(model: Model, rows, count: int = 2) -> list:
    """the first `count` of `rows` that are no cluster rows"""
    return [int(r) for r in rows if 0 <= r < len(model) and not model.tag[int(r)]][:count]


def edit(kind: Kind, model: Model, step: Step, seed: int) -> Edit:
    """The step as it applies to `model` (which is not changed).  Asserts what the step's name promises about `norm_rows`."""
    rng = np.random.default_rng(seed)
    n, nr, d = len(model), model.norm_rows, kind.dim
    new_rows = lambda m: make_corpus(m, d, seed + 7)[0]  # noqa: E731
    aimed: list = []

    def aim_rows(after: Model, what: str, rows, count: int = 2):
        for r in _plain(after, rows, count):
            aimed.append((what, seen(kind, after.raw[r]), r))

    if step.op == "append":
        m = 40
        rows, msgs = new_rows(m), rng.integers(0, ROWS // 3, size=m).astype(np.int64)
        grows = n + m > model.cap
        after = Model(np.concatenate([model.raw, rows]), np.concatenate([model.msgs, msgs]), np.concatenate([model.tag, np.zeros(m, np.int8)]),
                      0 if grows else nr, max(n + m, 2 * model.cap) if grows else model.cap)
        aim_rows(after, "new", [n, n + 1, n + m - 1, n + m - 2], 4)
        aim_rows(after, "front", [n - 1, 0])
        return Edit(step, "add_embeddings", {"rows": rows}, after, n, aimed, map_again=True)
    if step.op == "clear_add":
        after = Model(model.raw[::-1].copy(), model.msgs[::-1].copy(), model.tag[::-1].copy(), 0, model.cap)
        aim_rows(after, "moved", [0, 1, n // 2, n - 2, n - 1])
        return Edit(step, "clear_add", {"rows": after.raw}, after, 0, aimed, map_again=True)
    if step.op == "insert":
        m = 37
        if step.where == "front":
            at = np.int64(0)  # one position: every row goes in front of the first
        elif step.where == "middle":
            at = rng.integers(n // 4, 3 * n // 4, size=m)
            at[:3] = [at[3], at[3], -(n // 3)]  # equal positions keep their order; a negative one wraps
        elif step.where == "chunk_edge":
            assert n >= CHUNK
            at = np.minimum(np.arange(CHUNK - 18, CHUNK - 18 + m), n)
        else:  # "tail": the first hole at or above norm_rows
            assert 0 < nr < n, "the step needs a cold tail"
            at = rng.integers(nr, n + 1, size=m)
            at[0], at[1] = nr, n
        rows, msgs = new_rows(m), rng.integers(0, ROWS // 3, size=m).astype(np.int64)
        assert n + m <= model.cap
        pos = positions_of(at, n, m)
        first = int(pos.min())
        after = Model(np.insert(model.raw, at, rows, axis=0), np.insert(model.msgs, at, msgs), np.insert(model.tag, at, np.zeros(m, np.int8)),
                      nr if first >= nr else 0, model.cap)
        assert (step.where == "tail") == (first >= nr) and np.array_equal(after.raw[pos], rows)
        if step.where == "chunk_edge":
            assert pos.min() < CHUNK <= pos.max()
        aim_rows(after, "new", [int(pos[0]), int(pos[m // 2]), int(pos[-1]), int(pos.max())])
        aim_rows(after, "moved", [r for r in range(first + 1, first + 12) if r not in set(pos.tolist())])
        aim_rows(after, "moved", [n + m - 1, n + m - 2, n + m - 3])
        aim_rows(after, "front", [first - 1, first - 2, 0])
        return Edit(step, "insert_rows", {"at": at, "rows": rows, "msgs": msgs}, after, first, aimed)
    if step.op == "set":
        m = 29
        if step.where == "below":
            which = rng.choice(nr, size=m, replace=False).astype(np.int64)
            which[0], which[1] = nr - 1, 0
            which[2] = which[3]  # a duplicate: the last one wins
            which[4] -= n  # a negative ordinal wraps
        elif step.where == "above":
            assert 0 < nr < n - m, "the step needs a cold tail"
            which = (nr + rng.choice(n - nr, size=m, replace=False)).astype(np.int64)
            which[0], which[1] = nr, n - 1
        else:
            assert 0 < nr < n - m, "the step needs a cold tail"
            which = np.concatenate([rng.choice(nr, size=m // 2, replace=False), nr + rng.choice(n - nr, size=m - m // 2, replace=False)]).astype(np.int64)
            which[0], which[-1] = nr - 1, nr
        rows = new_rows(m)
        after = Model(model.raw.copy(), model.msgs, model.tag.copy(), nr, model.cap)
        after.raw[which] = rows
        after.tag[which] = 0
        wrapped = which % n
        first = int(wrapped.min())
        aim_rows(after, "new", [int(wrapped[0]), int(wrapped[1]), int(wrapped[-1]), int(wrapped[m // 2])])
        for r in _plain(model, [int(x) for x in wrapped[5:9]]):
            aimed.append(("old", seen(kind, model.raw[r]), -1))
        aim_rows(after, "moved", [r for r in range(first + 1, first + 12) if r not in set(wrapped.tolist())])
        aim_rows(after, "moved", [r for r in (n - 1, n - 2, n - 3, n - 4) if r not in set(wrapped.tolist())])
        aim_rows(after, "front", [first - 1, 0] if first > 0 else [])
        return Edit(step, "set_rows", {"which": which, "rows": rows}, after, first, aimed)
    assert step.op == "remove"
    flags = np.zeros(n, dtype=bool)
    if step.where == "before":  # every removed row below norm_rows; a block over the chunk edge where there is one
        top = min(nr, n)
        flags[rng.choice(top, size=30, replace=False)] = True
        if top > CHUNK + 3:
            flags[CHUNK - 5 : CHUNK + 3] = True
        else:
            flags[top // 2 : top // 2 + 8] = True
        flags[top - 1] = True
    elif step.where == "across":
        assert 20 < nr < n - 20, "the step needs a cold tail"
        flags[nr - 15 : nr + 15] = True
    else:
        assert 0 < nr < n - 12, "the step needs a cold tail"
        flags[nr + rng.choice(n - nr, size=12, replace=False)] = True
        flags[nr] = True
    gone = np.flatnonzero(flags)
    first = int(gone[0])
    assert (step.where == "after") == (first >= nr)
    after = Model(np.delete(model.raw, gone, axis=0), np.delete(model.msgs, gone), np.delete(model.tag, gone), nr if first >= nr else 0, model.cap)
    for r in _plain(model, [int(gone[0]), int(gone[len(gone) // 2]), int(gone[-1])], 3):
        aimed.append(("old", seen(kind, model.raw[r]), -1))
    aim_rows(after, "moved", range(first, first + 12))
    aim_rows(after, "moved", [len(after) - 1, len(after) - 2, len(after) - 3])
    aim_rows(after, "front", [first - 1, first - 2, 0])
    return Edit(step, "remove_rows", {"which": flags if seed % 2 else gone}, after, first, aimed)


def apply_edit(vb, e):
    """One edit through the class, on the device and on the CPU twin's host-only index alike."""
    a = e.args
    if e.call == "add_embeddings":
        vb.add_embeddings(None, a["rows"].copy())
    elif e.call == "clear_add":
        vb.clear()
        vb.add_embeddings(None, a["rows"].copy())
    elif e.call == "insert_rows":
        assert vb.insert_rows(a["at"], a["rows"], row_messages=a["msgs"]) == len(a["rows"])
    elif e.call == "set_rows":
        assert vb.set_rows(a["which"], a["rows"]) == len(set((np.asarray(a["which"]) % len(vb)).tolist()))
    else:
        gone = a["which"]
        assert vb.remove_rows(gone) == (int(gone.sum()) if gone.dtype == np.bool_ else len(set(gone.tolist())))
    if e.map_again:
        vb.set_row_messages(e.model.msgs)


def positions_of(at, n: int, m: int) -> np.ndarray:
    """np.insert's rule: where the m new rows stand among n + m"""
    a = np.asarray(at, dtype=np.int64).reshape(-1).copy()
    a[a < 0] += n
    if a.size == 1:
        return a[0] + np.arange(m, dtype=np.int64)
    order = np.argsort(a, kind="stable")
    a[order] += np.arange(m, dtype=np.int64)
    return a


def step_seed(case_kind: Kind, seq: Sequence, i: int) -> int:
    return case_kind.seed + 97 * SEQUENCES.index(SEQUENCE[seq.name] if seq.keep_host_copy else SEQUENCE["long"]) + 13 * i + 5


def replay(kind: Kind, seq: Sequence) -> list[Edit]:
    """the edits of a sequence, each over the model its predecessor left (the device-only twin of a sequence makes the same edits)"""
    model, out = start(kind), []
    for i, step in enumerate(seq.steps):
        e = edit(kind, model, step, step_seed(kind, seq, i))
        out.append(e)
        model = e.model
        e.norm_rows = model.norm_rows
        if step.lookups:  # the legs of the checkpoint end in a wide batch: every row is covered again
            model.norm_rows = len(model)
    return out


# ---- the queries of a checkpoint ---------------------------------------------------------------------------------------------------------------
def checkpoint_mask(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed + 1).random(n) < 0.5


def checkpoint_scopes(n: int, seed: int, count: int = 8) -> list[np.ndarray]:
    """overlapping scopes: thirds of the rows by residue, each widened by a random sixth; two queries share one object"""
    rng = np.random.default_rng(seed + 2)
    r = np.arange(n)
    scopes = [(r % 3 == i % 3) | (rng.random(n) < 1 / 6) for i in range(count)]
    scopes[5] = scopes[1]
    return scopes


def _gaps(scores: np.ndarray, ks) -> np.ndarray:
    """scores [rows, C] -> the smallest gap between rank k and rank k + 1 over ks, per column"""
    kmax = max(ks)
    if kmax >= scores.shape[0]:
        return np.zeros(scores.shape[1])
    top = -np.sort(np.partition(-scores, kmax, axis=0)[: kmax + 1], axis=0)
    return np.min(np.stack([top[k - 1] - top[k] for k in ks]), axis=0)


@dataclass
class Checkpoint:
    queries: np.ndarray  # float32 [NQ, dim]: the aimed queries first
    aimed: list  # (what, row of the model or -1) of queries[: len(aimed)]
    cluster: np.ndarray  # the cluster's query: the flagged leg's last
    mask: np.ndarray
    scopes: list
    large: np.ndarray  # the queries of the large-k leg [3, dim] (the first is aimed)
    sort: np.ndarray  # ... of the sort-all leg


def score32(v: np.ndarray, q: np.ndarray) -> np.ndarray:
    return np.clip((v @ np.asarray(q, dtype=np.float32).T + 1.0) / 2.0, 0.0, 1.0)


def build_checkpoint(kind: Kind, e: Edit, seed: int) -> Checkpoint:
    model = e.model
    v = seen(kind, model.raw)
    n = len(v)
    _, _, _, c, pool = base(kind)
    rng = np.random.default_rng(seed + 3)
    mask = checkpoint_mask(n, seed)
    scopes = checkpoint_scopes(n, seed)
    for _, _, r in e.aimed:  # the rows aimed at are allowed everywhere
        if r >= 0:
            mask[r] = True
            for s in scopes:
                s[r] = True
    tries = 6
    cands, owner = [], []
    for j, (_, a, _) in enumerate(e.aimed):
        for t in range(tries):
            g = rng.standard_normal(kind.dim).astype(np.float32)
            cands.append(_unit(a) if t == 0 else _unit(_unit(a) + 0.05 * g / np.linalg.norm(g)))
            owner.append(j)
    n_aimed = len(cands)
    cands = np.concatenate([np.stack(cands), pool]) if cands else pool.copy()
    s = score32(v, cands)  # [n, C]
    ok = (_gaps(s, (8, 25, 32)) > MARGIN) & (_gaps(s[mask], (8, 32)) > MARGIN)
    for j, (_, _, r) in enumerate(e.aimed):  # an aimed row leads its query by more than the margin
        if r >= 0:
            cols = [i for i in range(n_aimed) if owner[i] == j]
            rest = np.delete(s[:, cols], r, axis=0).max(axis=0)
            ok[cols] &= s[r, cols] - rest > MARGIN
    picked, aimed_out = [], []
    for j, (what, _, r) in enumerate(e.aimed):
        cols = [i for i in range(n_aimed) if owner[i] == j and ok[i]]
        if cols and len(picked) < 24:
            picked.append(cols[0])
            aimed_out.append((what, r))
    # the first eight also run under a scope of their own
    fill = [i for i in range(n_aimed, len(cands)) if ok[i]]
    order = picked + fill
    good = []
    for i in order:
        slot = len(good)
        if slot < 8 and not (_gaps(s[scopes[slot]][:, [i]], (8,))[0] > MARGIN):
            if i in picked:
                j = picked.index(i)
                picked.pop(j)
                aimed_out.pop(j)
            continue
        good.append(i)
        if len(good) == NQ:
            break
    assert len(good) == NQ, f"only {len(good)} queries pass the gaps: another seed"
    assert good[: len(picked)] == picked
    big = _gaps(s, (300,)) > MARGIN
    every = list(range(n_aimed, len(cands)))  # (these two legs have their own k: the whole pool is theirs)
    large = ([i for i in picked if big[i]][:1] + [i for i in every if big[i]])[:3]
    thr = min_score_of(LEG["sort-all"], kind)
    clear = np.abs(s - thr).min(axis=0) > MARGIN
    some = (s >= thr).sum(axis=0) >= 1
    sort = ([i for i in picked if clear[i]][:1] + [i for i in every if clear[i] and some[i]])[:3]
    assert len(large) == 3 and len(sort) == 3, (len(large), len(sort))
    return Checkpoint(cands[good], aimed_out, c.copy(), mask, scopes, cands[large], cands[sort])


@functools.lru_cache(maxsize=3)
def checkpoints(kind: Kind, seq_name: str):
    """-> [(edit, its checkpoint or None)] of a sequence (the device-only twin shares its sequence's)"""
    seq = SEQUENCE[seq_name]
    if not seq.keep_host_copy:
        return checkpoints(kind, "long")
    out = []
    for i, e in enumerate(replay(kind, seq)):
        out.append((e, build_checkpoint(kind, e, step_seed(kind, seq, i)) if e.step.lookups else None))
    return out


def leg_queries(leg: Leg, cp: Checkpoint) -> np.ndarray:
    if leg.name == "large-k":
        return cp.large
    if leg.name == "sort-all":
        return cp.sort
    if leg.planted:
        return np.concatenate([cp.queries[: leg.nq - 1], cp.cluster[None]])
    return cp.queries[: leg.nq]
