"""Model-based lifecycle tests (-m gpu): one long-lived GpuIndex per storage type driven through a seeded schedule of appends,
compactions, updates, shadow requests, per-row inputs and poisoned rows (tests/lifecycle_model.py), checked after every probed step
against float64 scores of the host model over ALL rows, against a fresh index over the model's matrix bit for bit (scores of every row,
the int8 pass's and the 5-bit plane's bound of every row, candidate counts, top-k indices and score bits), and for its bookkeeping.
What each schedule covers is asserted on the CPU by tests/test_lifecycle_inputs.py.  A failure names (case, seed, step), which
lifecycle_model.replay re-runs.  Then the HyperDB facade, single index and three logical shards on one GPU, against plain Python
lists."""
import copy
import time

import numpy as np
import pytest

import lifecycle_model as lm
from test_facade import expected_with_recency

pytestmark = pytest.mark.gpu

RUNS = [(case, seed) for case in lm.CASES for seed in lm.SEEDS]


@pytest.mark.parametrize("case,seed", RUNS)
def test_index_follows_the_model(case, seed):
    c = lm.CASES[case]
    t0 = time.perf_counter()
    counts = lm.run(case, seed)
    print(f"{case} seed {seed}: {len(lm.schedule(case, seed))} steps in {time.perf_counter() - t0:.1f} s, {counts}")
    assert counts["subset"] >= 1, "no call took the row list: set_subset was not under test"
    assert counts["unmasked_after_input"] >= 3, "bias, mask and row list are each dropped by a mutation and probed after it"
    if c["shadow"]:
        assert counts["shadow_calls"] >= 2 and counts["plane_calls"] >= 2, counts
        assert counts["bounds_after_mutation"] >= 2, counts


@pytest.mark.parametrize("case", [name for name, c in lm.CASES.items() if c["storage"] in ("float8", "int8", "float64")])
def test_storage_types_without_a_shadow_refuse_one(case):
    m = lm.Model(case, 1)
    ix = lm.open_index(case, m.V)
    try:
        with pytest.raises(NotImplementedError):
            ix.quantize("int8")
        assert ix.stat("quant_bytes") == 0
    finally:
        ix.close()


@pytest.mark.parametrize("name", lm.PINNED)
def test_pinned_reductions(name):
    """Reduced schedules of the library bugs the random walk (python tests/lifecycle_model.py STEPS SEED) found."""
    case, seed, steps = lm.pinned_schedule(name)
    lm.run(case, seed, steps=steps)


# ---- the facade ----------------------------------------------------------------------------------------------------------------------
D = 64
TAGS = ("a", "b", "c")
FACADE_METRICS = ("cosine_similarity", "dot_product", "hamming_distance")


class Lists:
    """HyperDB as plain Python lists: documents and the stored float16 rows, in document order."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.docs, self.V, self.next_id = [], np.zeros((0, D), dtype=np.float16), 0

    def make(self, m):
        docs = [{"id": self.next_id + i, "tag": TAGS[int(self.rng.integers(0, 3))], "rare": (self.next_id + i) % 40 == 0,
                 "timestamp": 1.7e9 + 3600.0 * (self.next_id + i)} for i in range(m)]
        self.next_id += m
        return docs, self.rng.standard_normal((m, D)).astype(np.float32)

    def add(self, docs, vectors):
        self.docs += copy.deepcopy(docs)
        self.V = np.concatenate([self.V, vectors.astype(np.float16)], axis=0)

    def remove(self, index):
        n = len(self.docs)
        gone = {i % n if i < 0 else i for i in np.atleast_1d(np.asarray(index)).tolist()}
        keep = [i for i in range(n) if i not in gone]
        self.docs = [self.docs[i] for i in keep]
        self.V = self.V[keep]

    def filters(self):
        n = len(self.docs)
        skip = min(7, n - 2)
        return [("none", None, np.ones(n, dtype=bool)),
                ("tag", [("metadata", {"tag": "b"})], np.array([d["tag"] == "b" for d in self.docs], dtype=bool)),
                ("rare", [("metadata", {"rare": True})], np.array([d["rare"] for d in self.docs], dtype=bool)),
                ("skip_doc", [("skip_doc", skip)], np.arange(n) >= skip)]


@pytest.mark.parametrize("seed", lm.SEEDS)
def test_facade_follows_plain_lists(seed):
    """devices=None and devices=[0, 0, 0] side by side: adds behind tombstones, removals by index, negative index and list, below
    the quarter rule and past it, every row of the middle shard (tombstoned, then compacted to an empty shard), an in-place metadata
    edit, emptying the database and refilling it.  After every step: four filters x three metrics against oracle.rank over the
    lists, the ids of the returned documents, size(), .vectors, and the two facades against each other."""
    from hyperdb import HyperDB
    from oracle import ranking_oracle as orc
    model = Lists(seed)
    rng = np.random.default_rng(100 + seed)
    Q = rng.standard_normal((4, D)).astype(np.float16)
    docs, vec = model.make(900)
    model.add(docs, vec)
    kw = dict(fp_precision="float16", metadata_keys=["timestamp", "tag", "rare"], cache_size=8)
    one = HyperDB(documents=copy.deepcopy(docs), vectors=vec, **kw)
    grp = HyperDB(documents=copy.deepcopy(docs), vectors=vec, devices=[0, 0, 0], **kw)
    dbs = (one, grp)
    assert [s.n for s in grp._index.shards] == [300, 300, 300]
    step = [0]

    def answer(db, q, filters, metric, **more):
        return db.query(q.copy(), top_k=10, filters=filters, metric=metric, **more)

    def check(what):
        where = f"step {step[0]} ({what})"
        step[0] += 1
        n = len(model.docs)
        for db in dbs:
            assert db.size() == n, where
            if n == 0:
                assert db.vectors is None and db._index is None, where
                with pytest.raises(Exception, match="database is empty"):
                    db.query(Q[0])
            else:
                assert np.array_equal(db.vectors, model.V), where
                assert db._index.n == n + db._dead.size, where
        if n == 0:
            return
        for name, filters, keep in model.filters():
            assert keep.sum() >= 2, (where, name)                 # (one document left is the reference's 2-D special case: not this test's)
            for mi, metric in enumerate(FACADE_METRICS):
                q = Q[(step[0] + mi) % len(Q)]
                oi, osc = orc.rank(model.V[keep], q.copy(), top_k=10, metric=metric)
                exact = orc.exact_scores(model.V, q, metric)
                got = [answer(db, q, filters, metric) for db in dbs]
                for res in got:
                    idx, sc = np.array([r[2] for r in res]), np.array([r[1] for r in res], dtype=np.float64)
                    assert keep[idx].all(), (where, name, metric)
                    assert [r[0]["id"] for r in res] == [model.docs[i]["id"] for i in idx], (where, name, metric)
                    if metric == "hamming_distance":
                        assert sc.tolist() == osc.tolist() and np.array_equal(exact[idx], sc), (where, name, metric)
                    else:
                        assert orc.same_result_modulo_ties(idx, sc, np.nonzero(keep)[0][oi], osc, 1e-3), (where, name, metric)
                a, b = got
                assert [r[2] for r in a] == [r[2] for r in b] and [r[1] for r in a] == [r[1] for r in b], (where, name, metric, "the two facades differ")

    def add(m):
        docs, vec = model.make(m)
        model.add(docs, vec)
        for db in dbs:
            db.add(copy.deepcopy(docs), vectors=vec)

    def remove(index):
        model.remove(index)
        for db in dbs:
            db.remove_document(index)

    check("fresh")
    remove(17)
    assert all(db._dead.tolist() == [17] for db in dbs)
    check("a single index: a tombstone")
    remove(-1)
    assert all(db._dead.tolist() == [17, 899] for db in dbs)
    check("a negative index")
    remove(rng.choice(len(model.docs), 40, replace=False).tolist())
    assert all(db._dead.size == 42 for db in dbs)                # below the quarter rule: tombstones only
    check("a list below the quarter rule")
    add(300)
    assert all(db._dead.size == 42 and db._index.n == 1200 for db in dbs)
    check("an add behind tombstones")
    add(1)
    check("an add of one")
    add(299)
    assert [s.n for s in grp._index.shards] == [300, 300, 900]
    check("the last shard grew")
    # one probe with both decays and a filter (expected_with_recency: the newest KEPT document normalises)
    _, filters, keep = model.filters()[1]
    for db in dbs:
        res = answer(db, Q[0], filters, "cosine_similarity", recency_bias=0.5, timestamp_key="timestamp")
        oi, osc = expected_with_recency(orc, model.V, model.docs, keep, Q[0].copy(), top_k=10, recency_bias=0.5, metric="cosine_similarity")
        assert orc.same_result_modulo_ties(np.array([r[2] for r in res]), np.array([r[1] for r in res]), oi, osc, 1e-3)
        assert max(r[1] for r in res) > 0.4 and [r[0]["id"] for r in res] == [model.docs[r[2]]["id"] for r in res]
    # every live row of the middle shard: 4 x dead <= rows, so they stay as tombstones and the shard's mask is all zero
    lo, hi = grp._index.bounds[1]
    live = grp._live_rows()
    middle = np.flatnonzero((live >= lo) & (live < hi)).tolist()
    remove(middle)
    assert all(db._dead.size == 42 + len(middle) and db._index.n == 1500 for db in dbs)
    alive = np.ones(1500, dtype=bool)
    alive[grp._dead] = False
    assert not alive[lo:hi].any() and grp._index.shards[1].n == 300
    check("every row of the middle shard, tombstoned")
    for i in range(0, len(model.docs), 37):                      # an in-place metadata edit ...
        for docs in (model.docs, one.documents, grp.documents):
            docs[i]["tag"] = "b"
    for db in dbs:
        db.invalidate_rows()                                     # ... that the cached masks learn of here
    check("invalidate_rows after an in-place edit")
    remove(rng.choice(len(model.docs), 60, replace=False).tolist())
    assert all(db._dead.size == 0 and db._index.n == len(model.docs) for db in dbs)
    assert [s.n for s in grp._index.shards][1] == 0 and [s.row_base for s in grp._index.shards][2] == grp._index.shards[0].n
    check("a compaction that leaves the middle shard empty")
    add(50)
    check("an add beside an empty shard")
    remove([-1, -2, -3])
    assert all(db._dead.size == 3 for db in dbs)
    check("negative indices in a list")
    remove(rng.choice(len(model.docs), 400, replace=False).tolist())
    assert all(db._dead.size == 0 for db in dbs)
    check("a list past the quarter rule: compaction")
    remove(list(range(len(model.docs))))
    check("every document removed")
    add(200)
    assert [s.n for s in grp._index.shards] == [66, 67, 67]
    check("refilled")
    remove([0, -1])
    add(30)
    assert all(db._dead.size == 2 for db in dbs)
    check("an add behind the tombstones of the refilled database")
    assert step[0] <= 30
