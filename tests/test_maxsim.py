"""Multi-vector queries on the GPU (hdb_maxsim_host): groups ranked by the sum over a set's vectors of each vector's best row.

Integer data (|x| <= 8, d = 64, dot product, |x(t, r)| <= 4096, sums <= 33 * 4096 < 2^24) are scored and summed exactly by every
arithmetic the library has, so those answers are compared for EQUALITY with an int64 model of the contract.  Float data are held to
the project's bands, summed over the set, against the float64 model (_native.maxsim_host)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D_INT = 64
T_INT = (1, 4, 5, 9, 33)                 # one call of five sets, 52 vectors
OFF_INT = np.concatenate([[0], np.cumsum(T_INT)]).astype(np.int32)
K_INT = (1, 10, 100)
NEG = np.iinfo(np.int64).min // 4        # the model's -inf: sums of 33 of them stay far below every real score
_cache = {}


# ------------------------------------------------------------------------------------------------ the model
def model_maxsim(S, off, groups, n_groups, k, eligible=None, bias=None):
    """S: [nv, n] int64 scores -> (group ids [ns, k] int64, scores [ns, k] float64), -1 / -inf padded.  The contract, in numpy."""
    ns = len(off) - 1
    ok = (groups >= 0) & (groups < n_groups)
    if eligible is not None:
        ok = ok & eligible
    gi = groups[ok]
    out_i = np.full((ns, k), -1, np.int64)
    out_s = np.full((ns, k), -np.inf, np.float64)
    for s in range(ns):
        total = np.zeros(n_groups, np.int64)
        dead = np.zeros(n_groups, bool)
        for v in range(off[s], off[s + 1]):
            x = S[v] if bias is None else S[v] + bias
            best = np.full(n_groups, NEG, np.int64)
            np.maximum.at(best, gi, x[ok])
            dead |= best == NEG
            total += np.where(best == NEG, 0, best)
        order = np.lexsort((np.arange(n_groups), -total))
        order = order[~dead[order]][:k]
        out_i[s, :len(order)] = order
        out_s[s, :len(order)] = total[order]
    return out_i, out_s


def _layouts(n, rng):
    runs = np.unique(np.repeat(np.arange(n), rng.integers(1, 9, size=n))[:n], return_inverse=True)[1].reshape(-1)
    long_runs = np.unique(np.repeat(np.arange(n), rng.integers(50, 301, size=n))[:n], return_inverse=True)[1].reshape(-1)
    return {                                       # name -> (ids, n_groups, non-decreasing by row)
        "runs": (runs, int(runs.max()) + 1, True),
        "long": (long_runs, int(long_runs.max()) + 1, True),
        "shuffled": (rng.permutation(runs), int(runs.max()) + 1, False),
        "one": (np.zeros(n, np.int64), 1, True),
        "each": (np.arange(n), n, True),
        "gaps": (long_runs * 3, int(long_runs.max()) * 3 + 40, True),      # n_groups beyond the largest id: empty groups inside and behind
    }


def _int_data(n):
    if ("int", n) not in _cache:
        rng = np.random.default_rng(n + 1)
        V = rng.integers(-8, 9, size=(n, D_INT)).astype(np.int64)
        Q = rng.integers(-8, 9, size=(int(OFF_INT[-1]), D_INT)).astype(np.int64)
        S = Q @ V.T
        layouts = _layouts(n, rng)
        expect = {(name, k): model_maxsim(S, OFF_INT, g, ng, k) for name, (g, ng, _) in layouts.items() for k in K_INT}
        for a in (V, Q, S):
            a.setflags(write=False)
        _cache[("int", n)] = (V, Q, S, layouts, expect)
    return _cache[("int", n)]


def _make_index(V, storage):
    from hyperdb._native import GpuIndex
    if storage == "float32":
        return GpuIndex(V.astype(np.float32))
    if storage == "float16":
        return GpuIndex(V.astype(np.float16))
    if storage == "bfloat16":
        return GpuIndex(torch.from_numpy(V.astype(np.float32)).to(torch.bfloat16).cuda())
    if storage == "float8":
        return GpuIndex(torch.from_numpy(V.astype(np.float32)).to(torch.float8_e4m3fn).cuda())
    if storage == "bits":
        return GpuIndex(np.packbits(V > 0, axis=1), storage="bits")
    return GpuIndex(V.astype(np.int8), storage="int8")


def _same(got, want, what):
    gi, gs = got
    wi, ws = want
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:4].tolist())
    assert np.array_equal(gs.astype(np.float64), ws), what


# ------------------------------------------------------------------------------------------------ exact equality on integer data
@pytest.mark.parametrize("n", [3_000, 20_001])
@pytest.mark.parametrize("storage", ["float32", "float16", "bfloat16", "float8", "int8", "bits"])
def test_integer_data_equal_the_model(storage, n):
    """Group ids and scores equal the int64 model on every storage, both sizes (at most 8192 rows; an odd tail above), the six
    layouts and k = 1, 10, 100; maxsim_sorted is 1 exactly for the layouts whose ids do not decrease."""
    from hyperdb._native import METRIC_IDS
    V, Q, S, layouts, expect = _int_data(n)
    if storage == "bits":                          # the rows are V > 0: a model of their own, same queries
        key = ("bits", n)
        if key not in _cache:
            Sb = Q @ (V > 0).astype(np.int64).T
            _cache[key] = {(name, k): model_maxsim(Sb, OFF_INT, g, ng, k) for name, (g, ng, _) in layouts.items() for k in K_INT}
        expect = _cache[key]
    ix = _make_index(V, storage)
    try:
        mid = METRIC_IDS["dot_product"]
        Qf = Q.astype(np.float32)
        for name, (g, ng, sorted_) in layouts.items():
            ix.set_groups(g, ng)
            for k in K_INT:
                _same(ix.maxsim(Qf, OFF_INT, k, mid), expect[(name, k)], (storage, n, name, k))
                assert ix.stat("maxsim") == 1 and ix.stat("grouped") == 0 and ix.stat("rerank") == 0
                assert ix.stat("maxsim_sorted") == (1 if sorted_ else 0), (name, ix.stat("maxsim_sorted"))
                assert ix.stat("path") == 2 and (ix.maxsim_status == 0).all()
            assert ix.stat("maxsim_bytes") >= 4 * (ng + 1) + (0 if sorted_ else 4 * n)
    finally:
        ix.close()


def test_chunks_cut_across_sets():
    """exact_bytes lowered to its floor of 1 MiB on 70 001 float32 rows: the plan is cq = 3 vectors per chunk, all five sets in one
    block, 18 chunks that cut across the set boundaries.  The arrays are those of the default plan (one chunk)."""
    from hyperdb._native import METRIC_IDS
    n = 70_001
    rng = np.random.default_rng(5)
    V = rng.integers(-8, 9, size=(n, D_INT)).astype(np.int64)
    Q = rng.integers(-8, 9, size=(int(OFF_INT[-1]), D_INT)).astype(np.int64)
    g, ng, _ = _layouts(n, rng)["long"]
    want = model_maxsim(Q @ V.T, OFF_INT, g, ng, 10)
    ix = _make_index(V, "float32")
    try:
        ix.set_groups(g, ng)
        one = ix.maxsim(Q.astype(np.float32), OFF_INT, 10, METRIC_IDS["dot_product"])
        assert ix.stat("maxsim_chunks") == 1
        _same(one, want, "one chunk")
        ix.set_option("exact_bytes", 1 << 20)
        cut = ix.maxsim(Q.astype(np.float32), OFF_INT, 10, METRIC_IDS["dot_product"])
        assert ix.stat("maxsim_chunks") == 18 and ix.stat("chunks") == 18
        _same(cut, want, "18 chunks")
        assert np.array_equal(cut[0], one[0]) and np.array_equal(cut[1], one[1])
    finally:
        ix.close()


@pytest.mark.parametrize("n", [3_000, 20_001])
def test_team_sizes_agree(n):
    from hyperdb._native import METRIC_IDS
    V, Q, S, layouts, expect = _int_data(n)
    ix = _make_index(V, "float16")
    try:
        for name in ("runs", "long", "shuffled", "one", "each", "gaps"):
            g, ng, _ = layouts[name]
            ix.set_groups(g, ng)
            for team in (1, 4, 16, 64):
                ix.set_option("maxsim_team", team)
                _same(ix.maxsim(Q.astype(np.float32), OFF_INT, 10, METRIC_IDS["dot_product"]), expect[(name, 10)], (n, name, team))
                assert ix.stat("maxsim_team") == team
            ix.set_option("maxsim_team", 0)
            ix.maxsim(Q.astype(np.float32), OFF_INT, 10, METRIC_IDS["dot_product"])
            assert ix.stat("maxsim_team") in (1, 4, 16, 64)
    finally:
        ix.close()


@pytest.mark.parametrize("storage,n", [("float32", 3_000), ("float16", 20_001), ("int8", 20_001)])
def test_mask_and_bias(storage, n):
    from hyperdb._native import METRIC_IDS
    V, Q, S, layouts, _ = _int_data(n)
    rng = np.random.default_rng(11)
    g, ng, _ = layouts["long"]
    mask = rng.random(n) < 0.6
    gone = rng.choice(ng, size=max(2, ng // 3), replace=False)       # every row of these groups is removed
    mask[np.isin(g, gone)] = False
    bias = rng.integers(-300, 301, size=n).astype(np.int64)
    ix = _make_index(V, storage)
    try:
        ix.set_groups(g, ng)
        ix.set_row_mask(mask)
        ix.set_bias(bias.astype(np.float32))
        for k in (10, ng):                                             # k = ng: beyond the eligible groups
            got = ix.maxsim(Q.astype(np.float32), OFF_INT, k, METRIC_IDS["dot_product"])
            _same(got, model_maxsim(S, OFF_INT, g, ng, k, eligible=mask, bias=bias), (storage, n, k))
            assert not np.isin(got[0], gone).any()
        assert (got[0][:, -1] == -1).all() and np.isneginf(got[1][:, -1]).all()
    finally:
        ix.close()


def test_matrix_cores_pinned():
    """float16, d = 128, 20 001 rows, one set of nine vectors: the score pass runs on the matrix cores; T = 1 on the same handle."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    rng = np.random.default_rng(3)
    n, d = 20_001, 128
    V = rng.integers(-8, 9, size=(n, d)).astype(np.int64)
    Q = rng.integers(-8, 9, size=(9, d)).astype(np.int64)
    g, ng, _ = _layouts(n, rng)["runs"]
    ix = GpuIndex(V.astype(np.float16))
    try:
        ix.set_groups(g, ng)
        off = np.array([0, 9], np.int32)
        got = ix.maxsim(Q.astype(np.float32), off, 10, METRIC_IDS["dot_product"])
        assert ix.stat("mfma") == 1 and ix.stat("maxsim") == 1
        _same(got, model_maxsim(Q @ V.T, off, g, ng, 10), "nine vectors")
        off1 = np.array([0, 1], np.int32)
        got = ix.maxsim(Q[:1].astype(np.float32), off1, 10, METRIC_IDS["dot_product"])
        _same(got, model_maxsim(Q[:1] @ V.T, off1, g, ng, 10), "one vector")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ float data
def _float_scores(V, q, metric):
    from hyperdb._native import _host_scores
    return _host_scores(V, q, metric)


@pytest.mark.parametrize("storage", ["float32", "float16"])
@pytest.mark.parametrize("metric", ["cosine_similarity", "euclidean_metric"])
def test_float_data_within_the_summed_bands(storage, metric):
    """Gaussian rows, sets of 9 and 33 vectors.  Every returned score is within B = sum_t tol * max(1, |x_t|) + (T - 1) 2^-24 sum_t |x_t|
    of the model's score of that group (tol: 1e-3 float16, 1e-5 otherwise), the j-th returned score within B of the model's j-th
    best, and no group appears twice."""
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(17)
    n, d, k = 20_001, 128, 20
    V = rng.standard_normal((n, d)).astype(np.float32)
    Vs = V.astype(np.float16) if storage == "float16" else V
    sets = [rng.standard_normal((9, d)).astype(np.float32), rng.standard_normal((33, d)).astype(np.float32)]
    off = np.array([0, 9, 42], np.int32)
    flat = np.concatenate(sets)
    g, ng, _ = _layouts(n, rng)["runs"]
    tol = 1e-3 if storage == "float16" else 1e-5
    ix = _make_index(Vs, storage)
    try:
        ix.set_groups(g, ng)
        gi, gs = ix.maxsim(flat, off, k, METRIC_IDS[metric])
    finally:
        ix.close()
    V64 = Vs.astype(np.float64)
    for s in range(2):
        terms = np.empty((off[s + 1] - off[s], ng))
        for j, v in enumerate(range(off[s], off[s + 1])):
            best = np.full(ng, -np.inf)
            np.maximum.at(best, g, _float_scores(V64, flat[v], metric))
            terms[j] = best
        total = terms.sum(axis=0)
        T = terms.shape[0]
        B = (tol * np.maximum(1.0, np.abs(terms))).sum(axis=0) + (T - 1) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
        ids = gi[s]
        assert (ids >= 0).all() and len(set(ids.tolist())) == k
        err = np.abs(gs[s].astype(np.float64) - total[ids])
        print(storage, metric, "T", T, "max error", err.max(), "band", B[ids].min())
        assert (err <= B[ids]).all(), (s, err.max(), B[ids].min())
        top = np.lexsort((np.arange(ng), -total))[:k]               # the model's k best: position j within B of the returned group
        assert (np.abs(gs[s].astype(np.float64) - total[top]) <= B[ids]).all()


@pytest.mark.parametrize("storage", ["float32", "float16"])
def test_euclidean_near_duplicates_within_the_summed_bands(storage):
    """Euclidean, 20 001 rows, sets of 5 and 9 vectors of which most are copies of rows (distance 0, score 1) or rows plus a
    perturbation of 1e-3: the rows a group's maximum picks.  ||v||^2 + ||q||^2 - 2 v.q would cancel there (about 1e-2 off); the call
    is held to the same summed band as every other float call, and its score pass does not take the matrix cores."""
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(31)
    n, d, k = 20_001, 128, 20
    V = rng.standard_normal((n, d)).astype(np.float32)
    Vs = V.astype(np.float16) if storage == "float16" else V
    V64 = Vs.astype(np.float64)
    rows = rng.choice(n, size=14, replace=False)
    flat = Vs[rows].astype(np.float32)                                # exact copies of stored rows ...
    flat[1::3] += (1e-3 * rng.standard_normal((len(flat[1::3]), d))).astype(np.float32)      # ... near-duplicates ...
    flat[4] = rng.standard_normal(d).astype(np.float32)               # ... and vectors that are neither
    flat[9] = rng.standard_normal(d).astype(np.float32)
    off = np.array([0, 5, 14], np.int32)
    g, ng, _ = _layouts(n, rng)["runs"]
    tol = 1e-3 if storage == "float16" else 1e-5
    ix = _make_index(Vs, storage)
    try:
        ix.set_groups(g, ng)
        gi, gs = ix.maxsim(flat, off, k, METRIC_IDS["euclidean_metric"])
        assert ix.stat("mfma") == 0 and ix.stat("maxsim") == 1
    finally:
        ix.close()
    for s in range(2):
        terms = np.empty((off[s + 1] - off[s], ng))
        for j, v in enumerate(range(off[s], off[s + 1])):
            best = np.full(ng, -np.inf)
            np.maximum.at(best, g, _float_scores(V64, flat[v], "euclidean_metric"))
            terms[j] = best
        total = terms.sum(axis=0)
        T = terms.shape[0]
        B = (tol * np.maximum(1.0, np.abs(terms))).sum(axis=0) + (T - 1) * 2.0 ** -24 * np.abs(terms).sum(axis=0)
        ids = gi[s]
        assert (ids >= 0).all() and len(set(ids.tolist())) == k
        assert set(g[rows[off[s]:off[s + 1]]].tolist()) & set(ids[:T].tolist())      # groups of copied rows lead the answer
        err = np.abs(gs[s].astype(np.float64) - total[ids])
        print(storage, "euclidean near-duplicates T", T, "max error", err.max(), "band", B[ids].min())
        assert (err <= B[ids]).all(), (s, err.max(), B[ids].min())
        top = np.lexsort((np.arange(ng), -total))[:k]
        assert (np.abs(gs[s].astype(np.float64) - total[top]) <= B[ids]).all()


# ------------------------------------------------------------------------------------------------ bad ids, lifecycle
def test_bad_ids_are_masked_and_reported():
    from hyperdb._native import METRIC_IDS, Q_BADROW, lib, _check
    n = 20_001
    V, Q, S, layouts, _ = _int_data(n)
    g, ng, _ = layouts["runs"]
    bad = g.copy()
    bad[[17, 12_345]] = [-3, ng + 5]
    ok = np.ones(n, bool)
    ok[[17, 12_345]] = False
    ix = _make_index(V, "float32")
    try:
        ix.set_groups(g, ng)                                           # the Python side's own state; the ids go in through ctypes
        dev = torch.from_numpy(bad.astype(np.int32)).cuda()
        _check(lib().hdb_index_set_groups(ix._h, ctypes.c_void_p(dev.data_ptr()), ng), "hdb_index_set_groups")
        got = ix.maxsim(Q.astype(np.float32), OFF_INT, 10, METRIC_IDS["dot_product"])
        assert ((ix.maxsim_status & Q_BADROW) != 0).all()
        assert ix.stat("maxsim_sorted") == 0                           # (the id -3 sorts behind every group: the rows are not in order)
        _same(got, model_maxsim(S, OFF_INT, g, ng, 10, eligible=ok), "bad ids")
    finally:
        ix.close()


def test_lifecycle_and_neighbouring_calls():
    from hyperdb._native import METRIC_IDS
    n = 20_001
    V, Q, S, layouts, expect = _int_data(n)
    mid = METRIC_IDS["dot_product"]
    Qf = Q.astype(np.float32)
    ix = _make_index(V, "float32")
    try:
        g1, ng1, _ = layouts["runs"]
        g2, ng2, _ = layouts["shuffled"]
        ix.set_groups(g1, ng1)
        plain0 = ix.topk(Qf[:4], 10, mid)
        grouped0 = ix.topk_grouped(Qf[:4], 10, mid)
        a = ix.maxsim(Qf, OFF_INT, 10, mid)
        _same(a, expect[("runs", 10)], "first ids")
        assert ix.stat("maxsim") == 1 and ix.stat("grouped") == 0
        # a grouped call and a plain top-k in between: their answers are what they were, and the stats follow the last call
        grouped1 = ix.topk_grouped(Qf[:4], 10, mid)
        assert ix.stat("maxsim") == 0 and ix.stat("grouped") == 1
        plain1 = ix.topk(Qf[:4], 10, mid)
        assert ix.stat("maxsim") == 0 and ix.stat("grouped") == 0
        for x, y in zip(plain0 + grouped0, plain1 + grouped1):
            assert np.array_equal(x, y)
        _same(ix.maxsim(Qf, OFF_INT, 10, mid), expect[("runs", 10)], "after the neighbours")
        assert ix.stat("maxsim") == 1 and ix.stat("maxsim_sorted") == 1
        # new ids: the next answer follows them
        ix.set_groups(g2, ng2)
        _same(ix.maxsim(Qf, OFF_INT, 10, mid), expect[("shuffled", 10)], "second ids")
        assert ix.stat("maxsim_sorted") == 0
        # append drops the ids
        ix.append(V[:3].astype(np.float32))
        with pytest.raises(ValueError, match="no groups set"):
            ix.maxsim(Qf, OFF_INT, 10, mid)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ the Python layers
def test_rank_maxsim():
    import hyperdb.ranking_algorithm as ranking
    rng = np.random.default_rng(23)
    n, d = 3_000, D_INT
    V = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    sets3 = rng.integers(-8, 9, size=(3, 4, d)).astype(np.float32)
    # groups=None: the rows ranked by their summed scores
    gi, gs = ranking.rank_maxsim(V, sets3, top_k=7, metric="dot_product")
    assert gi.dtype == np.int64 and gs.dtype == np.float64 and gi.shape == (3, 7)
    for s in range(3):
        total = (sets3[s].astype(np.int64) @ V.astype(np.int64).T).sum(axis=0)
        order = np.lexsort((np.arange(n), -total))[:7]
        assert np.array_equal(gi[s], order) and np.array_equal(gs[s], total[order].astype(np.float64))
    # the 3-D and the ragged-list inputs agree; one (T, d) array is one set
    groups = np.arange(n) // 7
    a = ranking.rank_maxsim(V, sets3, groups, top_k=5, metric="dot_product")
    b = ranking.rank_maxsim(V, [sets3[0], sets3[1], sets3[2]], groups, top_k=5, metric="dot_product")
    c = ranking.rank_maxsim(V, sets3[1], groups, top_k=5, metric="dot_product")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(c[0][0], a[0][1]) and c[0].shape == (1, 5)
    # top_k beyond n_groups is clamped
    few = np.arange(n) % 3
    gi, gs = ranking.rank_maxsim(V, sets3, few, top_k=50, metric="dot_product")
    assert gi.shape == (3, 3) and sorted(gi[0].tolist()) == [0, 1, 2]
    # a NaN raises
    bad = sets3.copy()
    bad[1, 2, 5] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        ranking.rank_maxsim(V, bad, groups)
    # a registered handle keeps no ids behind
    h = ranking.register_vectors(V)
    try:
        ranking.rank_maxsim(h, sets3, groups, top_k=5, metric="dot_product")
        assert h.index.n_groups == 0
    finally:
        h.close()


def test_query_multi_on_a_store():
    from hyperdb import HyperDB
    from hyperdb._native import maxsim_host
    rng = np.random.default_rng(29)
    n, d = 151, 32
    V = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    docs = [{"name": f"d{i}", "info": {"lang": "en" if i % 3 else "de"}} for i in range(n)]
    db = HyperDB(documents=docs, vectors=V, metadata_keys=["info.lang"])
    db.source_indices = [100 + i // 4 for i in range(n)]              # chunks of four documents share a source
    sources = np.asarray(db.source_indices)
    Q = rng.integers(-8, 9, size=(4, d)).astype(np.float32)
    for filters in (None, [("metadata", {"info.lang": "en"})]):
        keep = None if filters is None else np.array([doc["info"]["lang"] == "en" for doc in docs])
        codes = np.unique(sources, return_inverse=True)[1].reshape(-1)
        wi, ws = maxsim_host(V, Q, codes, 5, "dot_product", mask=keep)
        res = db.query_multi(Q, group_by="source", top_k=5, filters=filters, metric="dot_product")
        want_n = int((wi[0] >= 0).sum())
        assert len(res) == want_n
        for j, (key, score, members) in enumerate(res):
            in_group = np.flatnonzero(codes == wi[0, j])
            if keep is not None:
                in_group = in_group[keep[in_group]]
            assert key == sources[in_group[0]] and score == ws[0, j]
            assert members == [docs[i] for i in in_group]
        assert db.query_multi(Q, group_by="source", top_k=5, return_similarities=False, filters=filters, metric="dot_product") == [r[0] for r in res]
