"""Diverse top-k on the GPU: maximal marginal relevance over a call's candidates (hdb_mmr, hdb_mmr_host).

Integer data (|x| <= 8, dot product, dyadic lambda) make every float32 product, sum and val exact, so the whole pick sequence is
compared for equality with the numpy model of the contract, _native.mmr_host.  Real data are held to a greedy certificate: at every
step the GPU's pick, judged in float64 from the GPU's own earlier picks, reaches the best value within the project's float32 band."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STORAGES = ("int8", "float32", "float16", "bfloat16", "float8", "float64")
PAIRS = ("cosine_similarity", "dot_product", "euclidean_metric")
_cache = {}


def _make_index(V, storage, **kw):
    """-> (GpuIndex, the stored values as float64)."""
    from hyperdb._native import GpuIndex
    if storage == "float32":
        S = V.astype(np.float32)
        return GpuIndex(S, **kw), S.astype(np.float64)
    if storage == "float64":
        S = V.astype(np.float64)
        return GpuIndex(S, **kw), S
    if storage == "float16":
        S = V.astype(np.float16)
        return GpuIndex(S, **kw), S.astype(np.float64)
    if storage == "bfloat16":
        t = torch.from_numpy(V.astype(np.float32)).to(torch.bfloat16)
        return GpuIndex(t.cuda(), **kw), t.to(torch.float64).numpy()
    if storage == "float8":
        t = torch.from_numpy(V.astype(np.float32)).to(torch.float8_e4m3fn)
        return GpuIndex(t.cuda(), **kw), t.to(torch.float32).numpy().astype(np.float64)
    S = np.clip(np.rint(V), -128, 127).astype(np.int8)
    return GpuIndex(S, storage="int8", **kw), S.astype(np.float64)


def _ranked_lists(V, Q, m):
    """The top-m of every query by (dot product descending, row ascending), in int64: ids [nq, m], float32 scores."""
    S = Q.astype(np.int64) @ V.astype(np.int64).T
    rows = np.arange(V.shape[0])
    idx = np.stack([np.lexsort((rows, -S[q]))[:m] for q in range(S.shape[0])])
    return idx.astype(np.int64), np.take_along_axis(S, idx, axis=1).astype(np.float32)


def _int_case(d):
    """Integer rows and queries (n = 500, nq = 3) and, per (lambda, m, k), the model's answer: built once per d, shared by the storages."""
    from hyperdb._native import mmr_host
    if ("int", d) not in _cache:
        rng = np.random.default_rng(1000 + d)
        V = rng.integers(-8, 9, size=(500, d)).astype(np.int64)
        Q = rng.integers(-8, 9, size=(3, d)).astype(np.int64)
        cases = {}
        for m in (1, 5, 128, 257):
            idx, sc = _ranked_lists(V, Q, m)
            for lam in (0.0, 0.5, 0.75, 1.0):
                for k in sorted({1, m}):
                    cases[(lam, m, k)] = (idx, sc) + mmr_host(V, idx, sc, k, lam, "dot_product")
        _cache[("int", d)] = (V, cases)
    return _cache[("int", d)]


# ------------------------------------------------------------------------------------------------ 1. exact pick sequence
@pytest.mark.parametrize("storage,d", [(s, 64) for s in STORAGES] + [("float16", 100), ("float16", 384)])
def test_integer_data_equal_the_model(storage, d):
    """Ids, score bits and status equal the model for lambda 0 / 0.5 / 0.75 / 1, m 1 / 5 / 128 / 257 and k 1 / m on every storage;
    float16 also with 200-byte rows (the element loop) and d = 384 (three slices)."""
    from hyperdb._native import METRIC_IDS
    V, cases = _int_case(d)
    ix, _ = _make_index(V, storage)
    try:
        ties = 0
        for (lam, m, k), (idx, sc, wi, ws, wst) in cases.items():
            gi, gs, gst = ix.mmr_device(idx, sc, k, lam, METRIC_IDS["dot_product"])
            where = (storage, d, lam, m, k)
            assert np.array_equal(gi.cpu().numpy(), wi), (where, gi[0][:10].tolist(), wi[0][:10].tolist())
            assert np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)), where
            assert np.array_equal(gst.cpu().numpy(), wst), where
            assert ix.stat("mmr") == 1 and ix.stat("mmr_chunks") == 1
            if m == 128:
                ties += int((np.diff(sc[0]) == 0).sum())
        assert ties > 0          # (the lists hold relevance ties: the position rule is exercised)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 2. the whole range
def test_the_longest_list_is_a_complete_permutation():
    from hyperdb._native import METRIC_IDS, mmr_host
    rng = np.random.default_rng(7)
    V = rng.integers(-8, 9, size=(4096, 64)).astype(np.int64)
    Q = rng.integers(-8, 9, size=(1, 64)).astype(np.int64)
    idx, sc = _ranked_lists(V, Q, 2048)
    wi, ws, wst = mmr_host(V, idx, sc, 2048, 0.5, "dot_product")
    ix, _ = _make_index(V, "int8")
    try:
        gi, gs, gst = ix.mmr_device(idx, sc, 2048, 0.5, METRIC_IDS["dot_product"])
        gi = gi.cpu().numpy()
        assert sorted(gi[0].tolist()) == sorted(idx[0].tolist())
        assert np.array_equal(gi, wi) and np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and gst.tolist() == [0]
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 3. greedy certificate
def _pairs64(X, pm):
    if pm == "euclidean_metric":
        return np.stack([1.0 / (1.0 + np.sqrt(((X - x) ** 2).sum(axis=1))) for x in X])
    P = X @ X.T
    if pm == "cosine_similarity":
        nrm = np.linalg.norm(X, axis=1)
        P = P / (nrm[:, None] * nrm[None, :])
    return P


@pytest.mark.parametrize("d", [100, 384])
@pytest.mark.parametrize("storage", STORAGES)
def test_every_pick_is_greedy_within_the_float32_band(storage, d):
    """Gaussian rows, n = 3000, m = 256, k = 64, lambda 0.5, four queries, the three pair metrics.  For every step t, val is recomputed
    in float64 from the GPU's own earlier picks; the GPU's pick reaches max - tol, tol = 1e-5 * max(1, max|p|, max|r|)."""
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(31 * d)
    n, m, k, nq = 3000, 256, 64, 4
    V = rng.standard_normal((n, d)) * (20.0 if storage == "int8" else 1.0)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    ix, Vw = _make_index(V, storage)
    try:
        for pm in PAIRS:
            li, ls, _ = ix.topk_device(Q.astype(np.float64) if storage == "float64" else Q, m, METRIC_IDS[pm])
            gi, gs, gst = ix.mmr_device(li, ls, k, 0.5, METRIC_IDS[pm])
            li, ls, gi, gs = li.cpu().numpy(), ls.cpu().numpy(), gi.cpu().numpy(), gs.cpu().numpy()
            assert gst.tolist() == [0] * nq
            assert not np.array_equal(gi, li[:, :k]), (storage, d, pm)          # (not vacuous: diversity changed the answer)
            for q in range(nq):
                P = _pairs64(Vw[li[q]], pm)
                r = ls[q].astype(np.float64)
                tol = 1e-5 * max(1.0, np.abs(P).max(), np.abs(r).max())
                pos = {int(row): j for j, row in enumerate(li[q].tolist())}
                picked = []
                for t in range(k):
                    j = pos[int(gi[q, t])]
                    assert j not in picked and gs[q, t] == ls[q, j], (storage, d, pm, q, t)
                    val = r if t == 0 else 0.5 * r - 0.5 * P[:, picked].max(axis=1)
                    left = np.ones(m, bool)
                    left[picked] = False
                    short = val[left].max() - val[j]
                    assert short <= tol, (storage, d, pm, q, t, short, tol)
                    picked.append(j)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 4. list hygiene
def test_list_hygiene_on_the_device():
    from hyperdb._native import GpuIndex, METRIC_IDS, mmr_host, Q_BADROW, Q_NAN
    rng = np.random.default_rng(5)
    V = rng.integers(-8, 9, size=(40, 64)).astype(np.float32)
    V[7] = V[3]                                                  # an exact duplicate row
    ix = GpuIndex(V, row_base=1000)
    dot, cos = METRIC_IDS["dot_product"], METRIC_IDS["cosine_similarity"]
    far = 2 ** 40
    try:
        idx = np.array([[1000, -1, 1002, 1000, 1003, far + 5, 1004, 50, 999, 1040, 1039],      # padding, a repeat, -inf, outside ids
                        [-1] * 11,                                                           # all padding
                        [1005, -1, -1, 1006, -1, -1, -1, -1, -1, -1, -1],                    # fewer candidates than k
                        [far, far + 1, -far, 2 ** 62, 1001, 1001, 1001, 1001, 1001, 1001, 1001]], dtype=np.int64)
        sc = rng.integers(-50, 50, size=idx.shape).astype(np.float32)
        sc[0, 4] = -np.inf
        for lam in (0.0, 0.5, 1.0):
            wi, ws, wst = mmr_host(V, idx, sc, 4, lam, "dot_product", row_base=1000)
            gi, gs, gst = ix.mmr_device(idx, sc, 4, lam, dot)
            assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)), lam
            assert gst.tolist() == wst.tolist() == [Q_BADROW, 0, 0, Q_BADROW]
            assert wi[1].tolist() == [-1] * 4 and wi[2].tolist()[2:] == [-1, -1] and wi[3].tolist() == [1001, -1, -1, -1]
        # HDB_Q_NAN is carried over from the word that came in, every other bit is cleared
        _, _, gst = ix.mmr_device(idx, sc, 4, 0.5, dot, status=np.array([Q_NAN | 1, 2, Q_NAN, 1 | 2 | 16], np.int32))
        assert gst.tolist() == [Q_NAN | Q_BADROW, 0, Q_NAN, Q_BADROW]
        # exact duplicate rows with equal relevance: the lower position goes first; at lambda = 0 the copy goes last
        idx = np.array([[1010, 1007, 1011, 1003, 1012, 1013]], dtype=np.int64)
        sc = np.array([[1.0, 5.0, 2.0, 5.0, 3.0, 4.0]], dtype=np.float32)
        gi, _, _ = ix.mmr_device(idx, sc, 6, 1.0, cos)
        assert gi.tolist() == [[1007, 1003, 1013, 1012, 1011, 1010]]
        gi, _, _ = ix.mmr_device(idx, sc, 6, 0.0, cos)
        assert gi[0, 0].item() == 1007 and gi[0, 5].item() == 1003
        assert np.array_equal(gi.cpu().numpy(), mmr_host(V, idx, sc, 6, 0.0, "cosine_similarity", row_base=1000)[0])
        # sizes and lambda through the binding
        with pytest.raises(ValueError):
            ix.mmr_device(idx, sc, 7, 0.5, cos)
        with pytest.raises(ValueError):
            ix.mmr_device(idx, sc, 2, 1.5, cos)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 5. chunking
def test_chunks_answer_as_one_launch_does():
    from hyperdb._native import GpuIndex, METRIC_IDS
    rng = np.random.default_rng(11)
    V = rng.standard_normal((2000, 64)).astype(np.float32)
    Q = rng.standard_normal((5, 64)).astype(np.float32)
    ix = GpuIndex(V)
    cos = METRIC_IDS["cosine_similarity"]
    try:
        li, ls, _ = ix.topk_device(Q, 600, cos)
        a = [t.cpu().numpy() for t in ix.mmr_device(li, ls, 100, 0.5, cos)]
        assert ix.stat("mmr_chunks") == 1
        ix.set_option("exact_bytes", 1 << 20)                   # 608 x 608 x 4 bytes per query: one query per chunk
        b = [t.cpu().numpy() for t in ix.mmr_device(li, ls, 100, 0.5, cos)]
        assert ix.stat("mmr_chunks") == 5
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])
        assert not np.array_equal(a[0], li.cpu().numpy()[:, :100])
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ 6. one call equals its halves
def test_one_call_equals_its_halves():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(13)
    n, d, m, k = 3000, 96, 80, 20
    V = rng.standard_normal((n, d)).astype(np.float32)
    Q = rng.standard_normal((3, d)).astype(np.float32)
    ts = rng.uniform(0.0, 5.0, size=n)
    h = ranking.register_vectors(V)
    ix = h.index
    cos = METRIC_IDS["cosine_similarity"]
    try:
        mask = rng.random(n) < 0.5
        ix.set_row_mask(mask)
        ix.set_recency(ts, 0.3)
        gi, gs = ix.mmr(Q, m, k, cos, 0.5)
        assert ix.stat("mmr") == 1 and ix.stat("mmr_chunks") == 1 and ix.stat("rerank") == 0 and ix.stat("grouped") == 0
        li, ls, lst = ix.topk_device(Q, m, cos)
        assert ix.stat("mmr") == 0
        assert mask[li.cpu().numpy()].all()
        hi, hs, _ = ix.mmr_device(li, ls, k, 0.5, cos, status=lst)
        assert np.array_equal(gi, hi.cpu().numpy()) and np.array_equal(gs.view(np.uint32), hs.cpu().numpy().view(np.uint32))
        assert not np.array_equal(gi, li.cpu().numpy()[:, :k])
        ix.set_row_mask(None)
        ix.set_bias(None)
        # rank_mmr: the same halves with the recency it sets itself
        ri, rs = ranking.rank_mmr(h, Q, top_k=k, fetch_k=m, lambda_mult=0.5, timestamps=ts, recency_bias=0.3)
        ix.set_recency(ts, 0.3)
        li, ls, _ = ix.topk_device(Q, m, cos)
        hi, hs, _ = ix.mmr_device(li, ls, k, 0.5, cos)
        ix.set_bias(None)
        assert ri.dtype == np.int64 and rs.dtype == np.float64
        assert np.array_equal(ri, hi.cpu().numpy()) and np.array_equal(rs, hs.cpu().numpy().astype(np.float64))
        # lambda_mult = 1 is rank_batch
        for metric in ("cosine_similarity", "euclidean_metric", "manhattan_distance"):
            ri, rs = ranking.rank_mmr(h, Q, top_k=k, lambda_mult=1.0, metric=metric)
            bi, bs = ranking.rank_batch(h, Q, top_k=k, metric=metric)
            assert np.array_equal(ri, bi) and np.array_equal(rs, bs), metric
        # the default fetch_k is 4 top_k
        ri, _ = ranking.rank_mmr(h, Q, top_k=k)
        li, ls, _ = ix.topk_device(Q, 4 * k, cos)
        assert np.array_equal(ri, ix.mmr_device(li, ls, k, 0.5, cos)[0].cpu().numpy())
        # a raw matrix is registered for the call
        ri2, _ = ranking.rank_mmr(V, Q, top_k=k)
        assert np.array_equal(ri, ri2)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------ 7. composition
def test_rerank_and_two_stage_lists_compose():
    from hyperdb._native import GpuIndex, METRIC_IDS, mmr_host
    rng = np.random.default_rng(17)
    n, d = 2000, 64
    V = rng.integers(-8, 9, size=(n, d)).astype(np.int64)
    Q = rng.integers(-8, 9, size=(3, d)).astype(np.float32)
    dot = METRIC_IDS["dot_product"]
    second, _ = _make_index(V, "int8")
    first = GpuIndex(V > 0, storage="bits")
    try:
        cand = np.stack([rng.choice(n, size=60, replace=False) for _ in range(3)]).astype(np.int64)
        cand[0, 5] = -1
        li, ls, lst = second.rerank_device(Q, cand, 40, dot)
        gi, gs, gst = second.mmr_device(li, ls, 10, 0.5, dot, status=lst)
        wi, ws, wst = mmr_host(V, li.cpu().numpy(), ls.cpu().numpy(), 10, 0.5, "dot_product")
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gs.cpu().numpy(), ws) and gst.tolist() == wst.tolist()
        assert second.stat("mmr") == 1 and second.stat("rerank") == 0
        # a bits index as the first stage of a two-stage call, then MMR on the second handle
        ti, tsc = second.two_stage(first, Q, METRIC_IDS["cosine_similarity"], 200, Q, dot, 50)
        gi, gs, _ = second.mmr_device(ti, tsc, 12, 0.75, dot)
        wi, ws, _ = mmr_host(V, ti, tsc, 12, 0.75, "dot_product")
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gs.cpu().numpy(), ws)
        # ... and never on the bits handle itself
        with pytest.raises(NotImplementedError):
            first.mmr_device(ti, tsc, 12, 0.75, dot)
    finally:
        first.close()
        second.close()


# ------------------------------------------------------------------------------------------------ 8. behaviour
@pytest.mark.parametrize("seed", [0, 3])
def test_near_copies_do_not_fill_the_answer(seed):
    """Three clusters of 40 near copies around the query and 400 fillers: the plain top-3 is three rows of the closest cluster, the
    diverse top-3 one row of each cluster."""
    import hyperdb.ranking_algorithm as ranking
    rng = np.random.default_rng(seed)
    d = 64
    base = rng.standard_normal(d)
    rows, cluster = [], []
    for c, s in enumerate((0.3, 0.4, 0.5)):
        centre = base + s * rng.standard_normal(d)
        rows.append(centre + 0.02 * rng.standard_normal((40, d)))
        cluster += [c] * 40
    rows.append(rng.standard_normal((400, d)))
    cluster = np.asarray(cluster + [-1] * 400)
    V = np.concatenate(rows).astype(np.float32)
    order = rng.permutation(len(V))
    V, cluster = V[order], cluster[order]
    bi, _ = ranking.rank_batch(V, base[None, :], top_k=3)
    assert cluster[bi[0]].tolist() == [0, 0, 0]
    mi, ms = ranking.rank_mmr(V, base[None, :], top_k=3, fetch_k=120, lambda_mult=0.5)
    assert sorted(cluster[mi[0]].tolist()) == [0, 1, 2] and mi[0, 0] == bi[0, 0]


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals():
    import hyperdb.ranking_algorithm as ranking
    rng = np.random.default_rng(19)
    V = rng.standard_normal((300, 64)).astype(np.float32)
    Q = rng.standard_normal((2, 64)).astype(np.float32)
    bits = ranking.register_vectors(V > 0, storage="bits")
    try:
        with pytest.raises(NotImplementedError, match="bits"):
            ranking.rank_mmr(bits, Q, top_k=3)
    finally:
        bits.close()
    with pytest.raises(NotImplementedError, match="manhattan_distance"):
        ranking.rank_mmr(V, Q, top_k=3, pair_metric="manhattan_distance")
    with pytest.raises(ValueError):
        ranking.rank_mmr(V, Q, top_k=3, lambda_mult=-0.5)
    group = ranking.register_vectors(V, devices=[0, 0])
    try:
        with pytest.raises(NotImplementedError, match="one device"):
            ranking.rank_mmr(group, Q, top_k=3)
        with pytest.raises(NotImplementedError, match="one device"):
            ranking.rank_mmr(group.index, Q, top_k=3)
    finally:
        group.close()


# ------------------------------------------------------------------------------------------------ 10. facade
def test_query_diverse_on_a_store():
    from hyperdb import HyperDB
    from hyperdb._native import mmr_host
    rng = np.random.default_rng(23)
    n, d = 151, 32
    V = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
    V[20:30] = V[10:20]                                         # ten documents stored twice
    docs = [{"name": f"d{i}"} for i in range(n)]
    db = HyperDB(documents=docs, vectors=V)
    q = rng.integers(-8, 9, size=d).astype(np.float32)
    sources = list(db.source_indices)
    for filters, first in ((None, 0), ([("skip_doc", 25)], 25)):
        full = db.query(q, top_k=40, filters=filters, metric="dot_product")
        rows = np.array([[int(doc["name"][1:]) for doc, _, _ in full]], dtype=np.int64)
        rel = np.array([[s for _, s, _ in full]], dtype=np.float32)
        assert rows.min() >= first
        wi, ws, _ = mmr_host(V, rows, rel, 8, 0.5, "dot_product")
        res = db.query_diverse(q, top_k=8, fetch_k=40, lambda_mult=0.5, filters=filters, metric="dot_product")
        assert res == [(docs[r], float(s), sources[r]) for r, s in zip(wi[0].tolist(), ws[0].tolist())]
        assert [doc for doc, _, _ in res] != [doc for doc, _, _ in full[:8]]
        assert db.query_diverse(q, top_k=8, fetch_k=40, filters=filters, metric="dot_product", return_similarities=False) == [docs[r] for r in wi[0].tolist()]
        # lambda_mult = 1 is query()
        assert db.query_diverse(q, top_k=8, lambda_mult=1.0, filters=filters, metric="dot_product") == db.query(q, top_k=8, filters=filters, metric="dot_product")
    with pytest.raises(ValueError):
        db.query_diverse(q, top_k=8, lambda_mult=1.5)
