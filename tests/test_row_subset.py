"""Row-list scan (hdb_index_set_row_subset): a selective filter reads only the rows it keeps.

The contract: a call that takes the list returns the indices, float32 score bits and status words of the same call on a FRESH index
registered over V[rows] with bias[rows] and use_mfma = use_fused = use_quant = use_l1_tile = 0, indices mapped through rows; against
the masked call of the same handle it agrees modulo ties at the dtype's tolerance; a call that does not take the list is the masked
call bit for bit.  Every index here sets subset_min_n = 0 and subset_ratio = 1 unless the test is about the rule.
Base matrix: 60 001 Gaussian rows (not a multiple of 16); lists are random, ascending and contain row 0 and row n - 1."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 60_001
K = 10
LISTED = ("dot_product", "cosine_similarity", "euclidean_metric", "manhattan_distance", "pearson_correlation")
M_ALL = (5, 1000, 8192, 8193, 20_001)        # < k and one partial tile; a tail tile; the small path's last size; the sampled path's first; a strided list sample
_TORCH = {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
_CACHE = {}


def _matrix(dt, d):
    """The seeded base matrix as a host torch tensor of the stored dtype (one per (dtype, d), shared and never changed)."""
    key = ("V", dt, d)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 + d)
        _CACHE[key] = torch.from_numpy(rng.standard_normal((N, d))).to(_TORCH[dt]).contiguous()
    return _CACHE[key]


def _rows(m, n=N, seed=0):
    key = ("rows", m, n, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(77 + m + seed)
        inner = rng.choice(np.arange(1, n - 1), size=m - 2, replace=False)
        _CACHE[key] = np.sort(np.concatenate([[0, n - 1], inner])).astype(np.int64)
    return _CACHE[key]


def _mask(rows, n=N):
    mk = np.zeros(n, dtype=np.uint8)
    mk[rows] = 1
    return mk


def _queries(dt, d, nq, seed=5):
    rng = np.random.default_rng(seed + d)
    return rng.standard_normal((nq, d)).astype(np.float64 if dt == "f64" else np.float32)


def _bias(n=N):
    return np.random.default_rng(3).uniform(-0.5, 0.5, n).astype(np.float32)


def _index(dt, d):
    from hyperdb._native import GpuIndex
    ix = GpuIndex(_matrix(dt, d))
    ix.set_option("subset_min_n", 0)
    ix.set_option("subset_ratio", 1)
    return ix


def _fresh(dt, d, rows):
    """The contract's reference: a fresh index over V[rows], matrix cores, single launches, shadow and tile kernel off."""
    from hyperdb._native import GpuIndex
    ix = GpuIndex(_matrix(dt, d)[torch.from_numpy(rows)].contiguous())
    for name in ("use_mfma", "use_fused", "use_quant", "use_l1_tile"):
        ix.set_option(name, 0)
    return ix


def _call(ix, Q, metric, k=K, exact=False):
    from hyperdb._native import METRIC_IDS
    idx, sc, st = ix.topk_device(Q, k, METRIC_IDS[metric], exact=exact)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _mapped(idx, rows):
    return np.where(idx >= 0, rows[np.clip(idx, 0, len(rows) - 1)], -1)


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def _ulps(a, b):
    """Largest distance in float32 steps between two score arrays (same shape; equal infinities count as 0)."""
    ka, kb = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ka, kb = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka), np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    return int(np.abs(ka - kb).max()) if ka.size else 0


def _bit_equal_sweep(dt, d, metrics, nqs, biases, ms, exact_m=20_001):
    ix = _index(dt, d)
    bias = _bias()
    calls, misses = 0, []                    # every call is compared; the figures are printed before the assertion
    try:
        for m in ms:
            rows = _rows(m)
            fresh = _fresh(dt, d, rows)
            try:
                for with_bias in biases:
                    ix.set_bias(bias if with_bias else None)
                    fresh.set_bias(bias[rows] if with_bias else None)
                    ix.set_row_subset(_mask(rows), rows)
                    assert ix.stat("subset_rows") == m
                    for metric in metrics:
                        for nq in nqs:
                            Q = _queries(dt, d, nq)
                            for exact in ((False, True) if m == exact_m and nq == nqs[0] else (False,)):
                                got = _call(ix, Q, metric, exact=exact)
                                assert ix.stat("subset") == 1 and ix.stat("subset_rows") == m, (dt, d, m, metric, nq, exact)
                                path = ix.stat("path")
                                assert ix.stat("mfma") == 0 and ix.stat("fused") == 0 and ix.stat("quant") == 0
                                want = _call(fresh, Q, metric, exact=exact)
                                assert path == fresh.stat("path") == (0 if m <= 8192 else 2 if exact else 1), (dt, d, m, metric, nq, exact, path)
                                want = (_mapped(want[0], rows), want[1], want[2])
                                calls += 1
                                if not _same_bits(got, want):
                                    misses.append((m, metric, nq, with_bias, exact, "idx" if not np.array_equal(got[0], want[0]) else "",
                                                   "status" if not np.array_equal(got[2], want[2]) else "", f"{_ulps(got[1], want[1])} ulp"))
                                if m < K:
                                    assert (got[0][:, m:] == -1).all() and np.isneginf(got[1][:, m:]).all() and (got[0][:, :m] >= 0).all()
                                assert np.isin(got[0][got[0] >= 0], rows).all()
            finally:
                fresh.close()
    finally:
        ix.close()
    print(f"{dt} d={d} {metrics}: {len(misses)} of {calls} calls differ from the fresh compact index")
    for miss in misses[:20]:
        print("   ", miss)
    assert not misses, (dt, d, len(misses), calls, misses[:5])


# fp16 d = 384: one query takes the unrolled NJ = 3 kernel, four queries the four-query kernel, six are two query groups
@pytest.mark.parametrize("metric", LISTED)
@pytest.mark.parametrize("dt,d", [("f16", 384), ("f32", 96)])
def test_bits_of_the_fresh_compact_index_full_cross(dt, d, metric):
    _bit_equal_sweep(dt, d, (metric,), (1, 4, 6), (False, True), M_ALL)


# fp16 d = 200: 400-byte rows, ragged last step; d = 100: 200-byte rows, the generic kernel; bf16 d = 128; fp64 d = 40;
# float32 d = 384: 1536-byte rows, the unrolled NJ = 6 kernel of one query
@pytest.mark.parametrize("metric", LISTED)
@pytest.mark.parametrize("dt,d", [("f16", 200), ("f16", 100), ("bf16", 128), ("f64", 40), ("f32", 384)])
def test_bits_of_the_fresh_compact_index_metric_sweep(dt, d, metric):
    _bit_equal_sweep(dt, d, (metric,), (1, 6), (True,), M_ALL)


@pytest.mark.parametrize("dt,d,tol", [("f16", 384, 1e-3), ("f32", 96, 1e-5), ("bf16", 128, 1e-5), ("f64", 40, 1e-5)])
def test_against_the_masked_call(dt, d, tol):
    """Default options otherwise: a float16 index compares against the matrix-core path."""
    from oracle import ranking_oracle as orc
    ix = _index(dt, d)
    try:
        ix.set_bias(_bias())
        for m in (1000, 20_001):
            rows = _rows(m)
            ix.set_row_subset(_mask(rows), rows)
            for metric in ("cosine_similarity", "euclidean_metric"):
                for nq in (1, 6):
                    Q = _queries(dt, d, nq)
                    ix.set_option("use_subset", 1)
                    a = _call(ix, Q, metric)
                    assert ix.stat("subset") == 1
                    ix.set_option("use_subset", 0)
                    b = _call(ix, Q, metric)
                    assert ix.stat("subset") == 0 and ix.stat("subset_rows") == m
                    assert (a[2] == 0).all() and (b[2] == 0).all()
                    for q in range(nq):
                        assert orc.same_result_modulo_ties(a[0][q], a[1][q], b[0][q], b[1][q], tol), (dt, m, metric, nq, q)
    finally:
        ix.close()


def test_fallbacks_are_the_masked_call_bit_for_bit():
    dt, d, m = "f16", 384, 20_001
    rows = _rows(m)
    mask = _mask(rows)
    ix = _index(dt, d)
    try:
        ix.set_bias(_bias())

        def both(metric, k, nq=2, **opts):
            Q = _queries(dt, d, nq)
            for name, v in opts.items():
                ix.set_option(name, v)
            ix.set_row_subset(mask, rows)
            a = _call(ix, Q, metric, k=k)
            assert ix.stat("subset") == 0 and ix.stat("subset_rows") == m, (metric, k, opts)
            ix.set_row_mask(mask)
            assert ix.stat("subset_rows") == 0
            b = _call(ix, Q, metric, k=k)
            assert _same_bits(a, b), (metric, k, opts)
            return a

        both("hamming_distance", K)
        both("jaccard_similarity", K)
        both("cosine_similarity", 3000)                                   # a full sort inside: k > 2048 on more than 8192 listed rows
        both("cosine_similarity", K, subset_ratio=8)                      # 20 001 * 8 > 60 001
        ix.set_option("subset_ratio", 3)                                  # ... the rule is an inequality: 20 001 * 3 > 60 001, 20 000 * 3 is not
        ix.set_row_subset(_mask(rows[:-1]), rows[:-1])
        _call(ix, _queries(dt, d, 4), "cosine_similarity")
        assert ix.stat("subset") == 1
        _call(ix, _queries(dt, d, 5), "cosine_similarity")                # five queries are two passes
        assert ix.stat("subset") == 0
        both("cosine_similarity", K, subset_ratio=1, use_subset=0)
        both("cosine_similarity", K, use_subset=1, subset_min_n=10**9)
        ix.set_option("subset_min_n", 0)
        ix.set_row_subset(mask, rows)
        _call(ix, _queries(dt, d, 2), "cosine_similarity")
        assert ix.stat("subset") == 1                                     # (the switches are back: the list is taken again)
        # the measured rule never takes a matrix below 32 768 rows
        from hyperdb._native import GpuIndex
        small = GpuIndex(_matrix(dt, d)[:20_000].contiguous())
        try:
            r = _rows(200, n=20_000)
            small.set_row_subset(_mask(r, 20_000), r)
            _call(small, _queries(dt, d, 1), "cosine_similarity")
            assert small.stat("subset") == 0 and small.stat("subset_rows") == 200
        finally:
            small.close()
    finally:
        ix.close()


def test_lifecycle():
    dt, d, m = "f32", 96, 1000
    rows = _rows(m)
    mask = _mask(rows)
    Q = _queries(dt, d, 2)
    V = _matrix(dt, d)
    ix = _index(dt, d)
    try:
        def unmasked_next():
            assert ix.stat("subset_rows") == 0
            a = _call(ix, Q, "dot_product")
            assert ix.stat("subset") == 0
            ix.set_row_mask(None)
            b = _call(ix, Q, "dot_product")
            assert _same_bits(a, b) and not np.isin(a[0], rows).all()

        ix.set_row_subset(mask, rows)
        assert ix.stat("subset_rows") == m
        ix.append(V[:7])
        unmasked_next()
        ix.update(V)
        ix.set_row_subset(mask, rows)
        ix.update(V[:50_000].contiguous())
        unmasked_next()
        ix.update(V)
        ix.set_row_subset(mask, rows)
        ix.compact(np.arange(0, N, 2))
        unmasked_next()
        ix.update(V)
        ix.set_row_subset(mask, rows)
        ix.set_row_mask(None)                                   # clears both
        assert ix.stat("subset_rows") == 0
        ix.set_row_subset(mask, rows)
        ix.set_row_mask(mask)                                   # a new mask: no stale list beside it
        assert ix.stat("subset_rows") == 0
        _call(ix, Q, "dot_product")
        assert ix.stat("subset") == 0
        ix.set_row_subset(mask, torch.from_numpy(rows).to(ix.device))      # a resident list, and a second time (validated once)
        ix.set_row_subset(mask, ix._rows)
        _call(ix, Q, "dot_product")
        assert ix.stat("subset") == 1 and ix.stat("subset_rows") == m
        ix.set_row_subset(None, None)
        assert ix.stat("subset_rows") == 0
        # invalid lists: ValueError before anything reaches the library
        for bad in ([], rows[::-1].copy(), np.array([0, 5, 5, 9]), np.array([-1, 3]), np.array([3, N]), np.array([[1, 2]]), np.array([0.5, 2.5])):
            with pytest.raises(ValueError):
                ix.set_row_subset(mask, bad)
            assert ix.stat("subset_rows") == 0 and ix._rows is None
        with pytest.raises(ValueError):
            ix.set_row_subset(None, rows)
    finally:
        ix.close()


def test_host_call_reruns_a_failed_list_pass_over_the_list():
    """sample_target = 16 aims the sampled threshold at 16 survivors of the 20 001 listed rows: fewer than k = 100 pass, the status
    word says so on the list call and on the fresh index alike, and GpuIndex.topk (hdb_topk_host) re-runs exactly -- over the list."""
    from hyperdb._native import METRIC_IDS
    dt, d, m, k = "f32", 96, 20_001, 100
    rows = _rows(m)
    Q = _queries(dt, d, 3)
    ix, fresh = _index(dt, d), _fresh(dt, d, rows)
    try:
        ix.set_row_subset(_mask(rows), rows)
        for h in (ix, fresh):
            h.set_option("sample_target", 16)
        a = _call(ix, Q, "dot_product", k=k)
        b = _call(fresh, Q, "dot_product", k=k)
        assert ix.stat("subset") == 1 and (a[2] != 0).any() and np.array_equal(a[2], b[2])
        gi, gs = ix.topk(Q, k, METRIC_IDS["dot_product"])
        assert ix.stat("subset") == 1
        wi, ws = fresh.topk(Q, k, METRIC_IDS["dot_product"])
        assert np.array_equal(gi, rows[wi]) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        ei, es, est = _call(fresh, Q, "dot_product", k=k, exact=True)
        assert np.array_equal(wi, ei) and np.array_equal(ws.view(np.uint32), es.view(np.uint32))
    finally:
        ix.close()
        fresh.close()


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_facade_filters_take_the_list(devices):
    from hyperdb import HyperDB
    from oracle import ranking_oracle as orc
    rng = np.random.default_rng(21)
    n, d = 40_000, 128
    V = rng.standard_normal((n, d)).astype(np.float32).astype(np.float16)
    docs = [{"name": f"doc{i}", "info": {"type": f"t{i % 100}"}, "timestamp": 1.7e9 + 0.001 * i} for i in range(n)]
    db = HyperDB(documents=docs, vectors=V, fp_precision="float16", metadata_keys=["timestamp", "info.type"], cache_size=4, devices=devices)
    ts = np.array([x["timestamp"] for x in docs])
    ix = db._index
    ix.set_option("subset_min_n", 0)
    ix.set_option("subset_ratio", 1)
    shards = [sh for sh, lo, hi in db._shards()]
    took = lambda: [sh.stat("subset") for sh in shards]

    def check(filters, keep, top_k=10, **kw):
        q = rng.standard_normal(d).astype(np.float16)
        res = db.query(q, top_k=top_k, filters=filters, **kw)
        rb = kw.get("recency_bias", 0)
        first = rb * np.exp(ts[keep] - ts[keep].max()) if rb else None
        oi, osc = orc.rank(V[keep], q.copy(), top_k=top_k, metric="cosine_similarity", timestamps=first, recency_bias=rb)
        got_i, got_s = np.array([r[2] for r in res]), np.array([r[1] for r in res])
        assert orc.same_result_modulo_ties(got_i, got_s, np.nonzero(keep)[0][oi], osc, 1e-3), (filters[0][0], kw)

    one_in_100 = np.arange(n) % 100 == 7
    meta = [("metadata", {"info.type": "t7"})]
    three_hundred = np.zeros(n, dtype=bool)
    three_hundred[rng.choice(n, 300, replace=False)] = True
    for filters, keep in ((meta, one_in_100), ([("mask", three_hundred)], three_hundred)):
        for kw in ({}, {"recency_bias": 0.4, "timestamp_key": "timestamp"}):
            check(filters, keep, **kw)
            assert took() == [1] * len(shards), (filters[0][0], kw)
    passes = db.host_row_passes
    check(meta, one_in_100)                                       # a second query with the same filter: no host pass
    check(meta, one_in_100, recency_bias=0.4, timestamp_key="timestamp")
    assert db.host_row_passes == passes
    assert all(sh.stat("subset_rows") == 0 for sh in shards), "the list is cleared with the mask after every query"
    # three quarters of the rows: no list
    most = np.arange(n) % 4 != 0
    check([("mask", most)], most)
    assert took() == [0] * len(shards)
    # rows of the first half only: the second shard keeps none and gets a plain mask
    front = np.zeros(n, dtype=bool)
    front[rng.choice(n // 2, 250, replace=False)] = True
    check([("mask", front)], front)
    assert took()[0] == 1 and took()[1:] == [0] * (len(shards) - 1)
    # remove_document rebuilds list and mask together
    gone = np.nonzero(one_in_100)[0][:3].tolist()
    db.remove_document(gone)
    alive = np.ones(n, dtype=bool)
    alive[gone] = False
    q = rng.standard_normal(d).astype(np.float16)
    res = db.query(q, top_k=10, filters=meta)
    assert db.host_row_passes > passes and took()[0] == 1
    keep = one_in_100 & alive
    oi, osc = orc.rank(V[keep], q.copy(), top_k=10, metric="cosine_similarity")
    got_i = np.array([int(r[0]["name"][3:]) for r in res])         # (document numbers: removals shift the positions)
    assert not np.isin(got_i, gone).any()
    assert orc.same_result_modulo_ties(got_i, np.array([r[1] for r in res]), np.nonzero(keep)[0][oi], osc, 1e-3)
