"""GPU tests (-m gpu) of packed-bit storage (storage="bits", HDB_B1 = 10): np.packbits rows stay one bit per element on the device,
float32 queries meet them in hdb_bscan.hip (dot / cosine / pearson / euclidean / manhattan), and the bit metrics read the sign
cache, which for such a matrix is a re-layout of the rows.

References.  oracle/ranking_oracle.py (float64) on the float32 0/1 widening of the matrix, within the project's float32 contract:
1e-5 * max(1, |s|), hamming exact, jaccard 1e-6.  On 0/1 rows with unit-norm queries the float32 sum of a row stays under 0.2
band (checked on a CPU at d up to 1024), so whole score vectors are compared, not only the top rows.  Second reference: a
storage="int8" index over the same 0/1 values on the same device -- the same integers in a storage the project already has: the
bit metrics must return its indices and score bits, the other metrics agree within 1e-5 modulo ties.

Shapes: n = 20 003 (ragged last tile, many tiles per workgroup, sampled path), n = 300 (small path), n = 4 099 for the widest
rows; d = 32 (one word per row), 96 (12-byte rows: 4-byte pieces), 384, 1024 (two queries per pass) and 4128, past the last
table-resident cut of the QT rule (3840: the in-register fallback).  Matrices are rng.random((n, d)) < p, p = 0.5 and 0.1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "hamming_distance", "manhattan_distance",
           "jaccard_similarity", "pearson_correlation")
BIT_METRICS = ("hamming_distance", "jaccard_similarity")
N = 20_003
SHAPES = ((32, N, 0.5), (96, N, 0.5), (384, N, 0.5), (384, N, 0.1), (1024, 4_099, 0.5), (4128, 4_099, 0.5))


@pytest.fixture(scope="module")
def orc():
    from oracle import ranking_oracle
    return ranking_oracle


@pytest.fixture(scope="module")
def ranking():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import hyperdb.ranking_algorithm as r
    return r


def _tol(metric):
    return 0.0 if metric == "hamming_distance" else 1e-6 if metric == "jaccard_similarity" else TOL


_MATS, _QS, _REF = {}, {}, {}


def _matrix(d, n=N, p=0.5):
    """(bool bits [n, d], their float32 0/1 widening) per shape, shared by the tests and never modified."""
    key = (d, n, p)
    if key not in _MATS:
        rng = np.random.default_rng(1000 * d + n + int(100 * p))
        B = rng.random((n, d)) < p
        _MATS[key] = (B, B.astype(np.float32))
    return _MATS[key]


def _queries(d, nq=9):
    """Unit-norm Gaussian float32 queries per width."""
    if d not in _QS:
        Q = np.random.default_rng(77 + d).standard_normal((nq, d))
        _QS[d] = (Q / np.linalg.norm(Q, axis=1, keepdims=True)).astype(np.float32)
    return _QS[d]


def _exact(orc, d, n, p, metric, qi):
    """The float64 oracle's score vector of query qi of the width, computed once."""
    key = (d, n, p, metric, qi)
    if key not in _REF:
        _REF[key] = orc.exact_scores(_matrix(d, n, p)[1], _queries(d)[qi], metric)
    return _REF[key]


def _within(got, want, tol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    err = np.abs(got[fin] - want[fin])
    band = tol * np.maximum(1.0, np.abs(want[fin]))
    assert np.all(err <= band), f"error {err.max():.3e} at row {int(np.argmax(err - band))}, band {tol}"


def _bits_eq(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


# ------------------------------------------------------------------------------------------------
# 1. storage
# ------------------------------------------------------------------------------------------------
def test_storage_is_one_bit_per_element(ranking):
    import torch
    from hyperdb._native import GpuIndex, HDB_B1, pack_bits
    B, Bw = _matrix(96)
    for order in ("big", "little"):
        packed = np.packbits(B, axis=1, bitorder=order)
        assert np.array_equal(packed, pack_bits(Bw, order))
        for src in (packed, torch.from_numpy(packed), torch.from_numpy(packed).cuda(), B, torch.from_numpy(B)):
            ix = GpuIndex(src, storage="bits", bitorder=order)
            try:
                assert ix.dtype == HDB_B1 == 10 and ix.storage == "bits" and ix.bitorder == order
                assert ix.n == N and ix.d == 96
                assert ix.V.dtype == torch.uint8 and tuple(ix.V.shape) == (N, 12) and ix.V.element_size() * ix.V.numel() == N * 96 // 8
                host = ix.host_matrix()
                assert host.dtype == np.float32 and np.array_equal(host, Bw)
                hb = ix.host_bits()
                assert hb.dtype == np.uint8 and np.array_equal(hb, packed)
                assert not ix.has_nan
            finally:
                ix.close()
    with pytest.raises(ValueError, match="pack_bits"):
        GpuIndex(Bw[:10], storage="bits")
    with pytest.raises(ValueError, match="pack_bits"):
        GpuIndex(torch.from_numpy(Bw[:10]).cuda(), storage="bits")
    # without the keyword a uint8 array is still a float64 index
    ix = GpuIndex(np.packbits(B[:300], axis=1))
    try:
        assert ix.dtype == 2 and ix.V.dtype == torch.float64 and ix.d == 12
    finally:
        ix.close()
    h = ranking.register_vectors(np.packbits(B[:300], axis=1), storage="bits")
    try:
        got = np.asarray(ranking.dot_product(h, np.ones(96, dtype=np.float32)))
        assert got.dtype == np.float32 and np.array_equal(got, Bw[:300].sum(axis=1))
        assert h.shape == (300, 96)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 2. every bit at every position
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["big", "little"])
def test_every_bit_at_every_position(ranking, order):
    """One-hot queries: the dot product with e_j is column j of the matrix, exactly."""
    for d, picks in ((96, range(96)), (384, (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 127, 128, 255, 256, 382, 383)),
                     (1024, (0, 7, 8, 31, 32, 511, 512, 991, 992, 1015, 1016, 1023)), (4128, (0, 31, 32, 4095, 4096, 4127))):
        rng = np.random.default_rng(d)
        n = 1027
        B = rng.random((n, d)) < 0.5
        for r in range(n):                               # a walking one (and a zero behind it) over a random mask: every position is set in some row and clear in another
            B[r, (r * 5) % d] = True
            B[r, (r * 5 + 1) % d] = False
        wide = B.astype(np.float32)
        h = ranking.register_vectors(np.packbits(B, axis=1, bitorder=order), storage="bits", bitorder=order)
        try:
            for j in picks:
                q = np.zeros(d, dtype=np.float32)
                q[j] = 1.0
                got = np.asarray(ranking.dot_product(h, q))
                assert got.dtype == np.float32 and got.shape == (n,) and np.array_equal(got, wide[:, j]), (d, j)
        finally:
            h.close()


# ------------------------------------------------------------------------------------------------
# 3. full score vectors
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d,n,p", SHAPES)
def test_full_score_vectors(orc, ranking, d, n, p, metric):
    from hyperdb._native import METRIC_IDS
    B, Bw = _matrix(d, n, p)
    Q = _queries(d)
    fn = getattr(ranking, metric)
    h = ranking.register_vectors(np.packbits(B, axis=1), storage="bits")
    try:
        ix, mid, tol = h.index, METRIC_IDS[metric], _tol(metric)
        full = []
        for qi in range(3):
            got = np.asarray(fn(h, Q[qi].copy()))
            assert got.shape == (n,)
            _within(np.where(np.isnan(got.astype(np.float64)), -np.inf, got.astype(np.float64)), _exact(orc, d, n, p, metric, qi), tol)
            full.append(ix.scores(Q[qi], mid).cpu().numpy())
        if metric == "euclidean_metric":                 # ... and the raw distance
            dist = np.asarray(ranking.euclidean_metric(h, Q[0], get_similarity_score=False))
            _within(dist, orc.exact_scores(Bw, Q[0], "euclidean_metric") ** -1.0 - 1.0, TOL)
        # batches: 1 / 3 / 4 / 5 / 9 queries per call meet 1, 4, 4, 4 + 1 and 4 + 4 + 1 queries per pass (fewer on wide rows); every
        # returned score is the score vector's own float32 and the rows are a valid top-k of the oracle's vector
        k = 40
        for nq in (1, 3, 4, 5, 9):
            gi, gs = ix.topk(Q[:nq], k, mid)
            for qi in range(nq):
                orc.check_topk(gi[qi], gs[qi], Bw, Q[qi], metric, k, tol=tol, exact=_exact(orc, d, n, p, metric, qi))
                if qi < 3:
                    want = np.where(np.isnan(full[qi]), -np.inf, full[qi])[gi[qi]] + np.float32(0.0)
                    assert _bits_eq(gs[qi], want), (nq, qi)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 4. top-k through the pipelines, beside an int8 index over the same 0/1 values
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    from hyperdb._native import GpuIndex
    B, Bw = _matrix(384)
    b1 = GpuIndex(np.packbits(B, axis=1), storage="bits")
    i8 = GpuIndex(B.astype(np.int8), storage="int8")
    yield b1, i8, Bw
    b1.close()
    i8.close()


def _agree(orc, b1, i8, Q, k, metric, tag, exact=False, ref=None, path=None, biased=False):
    """biased: a float32 bias was added to the score in float32.  A hamming score is an integer up to d = 384, so that one addition
    rounds by up to half an ulp of 256 .. 512, 1.5e-5: hamming is exact only without a bias, with one it gets the float32 band."""
    from hyperdb._native import METRIC_IDS
    mid = METRIC_IDS[metric]
    tol = TOL if (biased and metric == "hamming_distance") else _tol(metric)
    gi, gs, gst = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid, exact=exact))
    stats = {s: b1.stat(s) for s in ("mfma", "quant", "plane", "subset", "fused", "path")}
    wi, ws, wst = (t.cpu().numpy() for t in i8.topk_device(Q, k, mid, exact=exact))
    assert stats["mfma"] == stats["quant"] == stats["plane"] == stats["subset"] == 0 and stats["fused"] in (0, 3), (tag, stats)
    if path is not None:
        assert stats["path"] == path, (tag, stats)
    assert (gst == 0).all(), (tag, gst)
    for qi in range(Q.shape[0]):
        if metric in BIT_METRICS:
            assert np.array_equal(gi[qi], wi[qi]) and _bits_eq(gs[qi], ws[qi]), (tag, qi)
        else:
            assert orc.same_result_modulo_ties(gi[qi], gs[qi], wi[qi], ws[qi], TOL), (tag, qi)
        if ref is not None:
            _check(orc, gi[qi], gs[qi], ref[qi], k, tol)
    if metric in BIT_METRICS:
        assert stats["fused"] == i8.stat("fused") and stats["path"] == i8.stat("path"), (tag, stats)
    return gi, gs


def _check(orc, idx, sc, exact, k, tol):
    """check_topk against a precomputed float64 score vector (bias and mask already in it)."""
    orc.check_topk(idx, sc, np.zeros((exact.shape[0], 1), dtype=np.float32), None, "dot_product", k, tol=tol, exact=exact)


@pytest.mark.parametrize("metric", METRICS)
def test_topk_through_the_pipelines(orc, pair, metric):
    b1, i8, Bw = pair
    d, n, p = 384, N, 0.5
    Q = _queries(d)[:3]
    ref = [_exact(orc, d, n, p, metric, qi) for qi in range(3)]
    rng = np.random.default_rng(11)
    bias = rng.uniform(-0.05, 0.05, n).astype(np.float32)
    mask = (rng.random(n) < 1.0 / 3.0).astype(np.uint8)
    try:
        for k in (10, 100):
            _agree(orc, b1, i8, Q, k, metric, ("sampled", k), ref=ref)
            _agree(orc, b1, i8, Q[:1], k, metric, ("sampled one", k), ref=ref[:1])
        _agree(orc, b1, i8, Q, 100, metric, "exact", exact=True, ref=ref, path=2)
        for ix in (b1, i8):
            ix.set_option("force_exact", 1)
        _agree(orc, b1, i8, Q, 100, metric, "force_exact", ref=ref, path=2)
        for ix in (b1, i8):
            ix.set_option("force_exact", 0)
        _agree(orc, b1, i8, Q[:2], 3000, metric, "full sort", ref=ref[:2], path=3)
        for ix in (b1, i8):
            ix.set_bias(bias)
        rb = [r + bias.astype(np.float64) for r in ref]
        _agree(orc, b1, i8, Q, 100, metric, "bias", ref=rb, biased=True)
        for ix in (b1, i8):
            ix.set_row_mask(mask)
        rbm = [np.where(mask != 0, r, -np.inf) for r in rb]
        gi, _ = _agree(orc, b1, i8, Q, 100, metric, "bias + mask", ref=rbm, biased=True)
        assert mask[gi].all()
        for ix in (b1, i8):
            ix.set_bias(None)
            ix.set_row_mask(mask)
        rm = [np.where(mask != 0, r, -np.inf) for r in ref]
        gi, _ = _agree(orc, b1, i8, Q, 100, metric, "mask", ref=rm)
        assert mask[gi].all()
    finally:
        for ix in (b1, i8):
            ix.set_option("force_exact", 0)
            ix.set_bias(None)
            ix.set_row_mask(None)


@pytest.mark.parametrize("metric", METRICS)
def test_small_path(orc, metric):
    from hyperdb._native import GpuIndex
    d, n = 96, 300
    B, Bw = _matrix(d, n)
    Q = _queries(d)[:5]
    b1 = GpuIndex(np.packbits(B, axis=1, bitorder="little"), storage="bits", bitorder="little")
    i8 = GpuIndex(B.astype(np.int8), storage="int8")
    try:
        ref = [orc.exact_scores(Bw, Q[qi], metric) for qi in range(5)]
        for k in (10, 300):
            _agree(orc, b1, i8, Q, k, metric, ("small", k), ref=ref, path=0)
    finally:
        b1.close()
        i8.close()


# ------------------------------------------------------------------------------------------------
# 5. near-row queries: the sum is over the per-element terms (||q||^2 + pop - 2 q.b misses the band by two orders of magnitude here)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [96, 384, 1024, 4128])
def test_near_row_queries(orc, ranking, d):
    n = 4_099
    B, Bw = _matrix(d, n)
    r = n - 2                                            # a row of the ragged last tile
    h = ranking.register_vectors(np.packbits(B, axis=1), storage="bits")
    try:
        for metric in ("euclidean_metric", "manhattan_distance"):
            got = np.asarray(getattr(ranking, metric)(h, Bw[r].copy()))
            assert got[r] == 1.0 and (np.delete(got, r) < 1.0).all(), metric
            idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, Bw[r].copy(), top_k=5, metric=metric)
            assert idx[0] == r and sc[0] == 1.0, metric
        q = (Bw[r] + np.random.default_rng(d).normal(0.0, 1e-3, d)).astype(np.float32)
        for metric in ("euclidean_metric", "manhattan_distance", "dot_product", "cosine_similarity", "pearson_correlation"):
            got = np.asarray(getattr(ranking, metric)(h, q.copy()))
            _within(got, orc.exact_scores(Bw, q, metric), TOL)
        dist = np.asarray(ranking.euclidean_metric(h, q.copy(), get_similarity_score=False))
        _within(dist, np.sqrt(((Bw.astype(np.float64) - q.astype(np.float64)) ** 2).sum(axis=1)), TOL)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 6. one arithmetic: a row's score bits are the same in every mode, pipeline and grid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_one_arithmetic(pair, metric):
    from hyperdb._native import METRIC_IDS
    b1, _, _ = pair
    mid = METRIC_IDS[metric]
    Q = _queries(384)[:5]
    bias = np.random.default_rng(12).uniform(-0.05, 0.05, N).astype(np.float32)
    k = 60
    try:
        for with_bias in (False, True):
            b1.set_bias(bias if with_bias else None)
            gi, gs, _ = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid))
            ei, es, _ = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid, exact=True))
            assert np.array_equal(gi, ei) and _bits_eq(gs, es), with_bias
            for qi in range(5):
                full = b1.scores(Q[qi], mid).cpu().numpy()
                want = full[gi[qi]] + (bias[gi[qi]] if with_bias else np.float32(0.0))
                assert _bits_eq(gs[qi], want.astype(np.float32)), (with_bias, qi)
            for blocks in (1, 64):
                b1.set_option("max_blocks", blocks)
                for exact in (False, True):
                    mi, ms, _ = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid, exact=exact))
                    assert np.array_equal(mi, gi) and _bits_eq(ms, gs), (with_bias, blocks, exact)
                b1.set_option("max_blocks", 0)
    finally:
        b1.set_option("max_blocks", 0)
        b1.set_bias(None)


# ------------------------------------------------------------------------------------------------
# 7. edge rows
# ------------------------------------------------------------------------------------------------
def test_all_zero_and_all_one_rows(orc, ranking):
    d, n = 96, 300
    B = _matrix(d, n)[0].copy()
    B[0] = False
    B[1] = True
    Bw = B.astype(np.float32)
    pop = B.sum(axis=1)
    q = _queries(d)[0]
    h = ranking.register_vectors(np.packbits(B, axis=1), storage="bits")
    try:
        cos = np.asarray(ranking.cosine_similarity(h, q.copy()))
        assert cos[0] == 0.0
        _within(cos, orc.exact_scores(Bw, q, "cosine_similarity"), TOL)
        pear = np.asarray(ranking.pearson_correlation(h, q.copy()))
        assert np.isnan(pear[0]) and np.isnan(pear[1]) and not np.isnan(pear[2:]).any()      # constant rows: the reference's NaN rule
        _within(np.where(np.isnan(pear), -np.inf, pear), orc.exact_scores(Bw, q, "pearson_correlation"), TOL)
        zero, one = np.zeros(d, dtype=np.float32), np.ones(d, dtype=np.float32)
        assert np.array_equal(np.asarray(ranking.hamming_distance(h, zero.copy())).astype(np.int64), d - pop)
        assert np.array_equal(np.asarray(ranking.hamming_distance(h, one.copy())).astype(np.int64), pop)
        jac = np.asarray(ranking.jaccard_similarity(h, zero.copy()))
        assert np.isnan(jac[0]) and np.array_equal(jac[1:], np.zeros(n - 1))                 # 0/0 -> NaN like numpy, 0/pop -> 0
        idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, zero.copy(), top_k=n, metric="jaccard_similarity")
        assert idx[-1] == 0 and sc[-1] == -np.inf and (sc[:-1] == 0.0).all()                   # ... and -inf in ranking: last
        idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, q.copy(), top_k=n, metric="pearson_correlation")
        assert set(idx[-2:].tolist()) == {0, 1} and (sc[-2:] == -np.inf).all()
        jac1 = np.asarray(ranking.jaccard_similarity(h, one.copy()))
        _within(jac1, pop / float(d), 1e-6)
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 8. lifecycle
# ------------------------------------------------------------------------------------------------
def _same_as_fresh(ix, rows_bool, tag):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    assert ix.n == rows_bool.shape[0] and np.array_equal(ix.host_matrix(), rows_bool.astype(np.float32)), tag
    assert np.array_equal(ix.host_bits(), np.packbits(rows_bool, axis=1, bitorder=ix.bitorder)), tag
    Q = _queries(ix.d)[:3]
    fresh = GpuIndex(rows_bool, storage="bits", bitorder=ix.bitorder)
    try:
        for metric in METRICS:
            gi, gs, gst = ix.topk_device(Q, 10, METRIC_IDS[metric])
            wi, ws, wst = fresh.topk_device(Q, 10, METRIC_IDS[metric])
            assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), (tag, metric)
    finally:
        fresh.close()


@pytest.mark.parametrize("d,order", [(32, "big"), (96, "little"), (384, "big")])
def test_lifecycle(d, order):
    from hyperdb._native import GpuIndex, METRIC_IDS
    rng = np.random.default_rng(d)
    rows = rng.random((9_000, d)) < 0.5
    pk = lambda b: np.packbits(b, axis=1, bitorder=order)
    ix = GpuIndex(pk(rows[:700]), storage="bits", bitorder=order)
    try:
        ham = METRIC_IDS["hamming_distance"]
        ix.topk(_queries(d)[:1], 5, ham)                  # the sign cache exists before the matrix grows
        ix.append(pk(rows[700:1500]))                     # packed rows; the allocation grows (rebase)
        q = rows[1400].astype(np.float32)
        gi, gs = ix.topk(q.reshape(1, -1), 1, ham)
        assert gs[0][0] == d and np.array_equal(rows[gi[0][0]], rows[1400])      # hamming sees the appended rows (the lazy sign cache)
        _same_as_fresh(ix, rows[:1500], "append packed")
        ix.append(rows[1500:1503])                        # bool rows
        _same_as_fresh(ix, rows[:1503], "append bool")
        for bad in (rows[:2].astype(np.float32), rows[:2].astype(np.int64), pk(rows[:2])[:, :-1], pk(rows[0:1])[0]):
            with pytest.raises(ValueError):
                ix.append(bad)
        _same_as_fresh(ix, rows[:1503], "a refused append stores nothing")
        keep = np.sort(rng.choice(1503, size=900, replace=False))
        ix.compact(keep)
        _same_as_fresh(ix, rows[:1503][keep], "compact")
        ix.append(pk(rows[1503:9000]))                    # growth past 8192 rows: small -> sampled, another rebase
        now = np.concatenate([rows[:1503][keep], rows[1503:9000]])
        _same_as_fresh(ix, now, "growth")
        ix.update(pk(rows[100:400]))
        _same_as_fresh(ix, rows[100:400], "update packed")
        ix.update(rows[50:99])
        _same_as_fresh(ix, rows[50:99], "update bool")
        with pytest.raises(ValueError):
            ix.update(rows[:5].astype(np.float32))
        _same_as_fresh(ix, rows[50:99], "a refused update stores nothing")
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 9. packed queries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["big", "little"])
def test_packed_query_equals_its_unpacked_form(ranking, order):
    import torch
    d = 384
    B, Bw = _matrix(d)
    rng = np.random.default_rng(9)
    qb = rng.random((5, d)) < 0.5
    qp = np.packbits(qb, axis=1, bitorder=order)
    qf = qb.astype(np.float32)
    h = ranking.register_vectors(np.packbits(B, axis=1, bitorder=order), storage="bits", bitorder=order)
    try:
        for metric in BIT_METRICS:
            fn = getattr(ranking, metric)
            keep = qp[0].copy()
            got = np.asarray(fn(h, qp[0]))
            assert np.array_equal(qp[0], keep)            # a packed query is bytes: never binarised in place
            assert np.array_equal(got, np.asarray(fn(h, qf[0].copy()))), metric
            assert np.array_equal(np.asarray(fn(h, torch.from_numpy(qp[0]).cuda())), got), metric
            i1, s1 = ranking.hyperDB_ranking_algorithm_sort(h, qp[0], top_k=20, metric=metric)
            i2, s2 = ranking.hyperDB_ranking_algorithm_sort(h, qf[0].copy(), top_k=20, metric=metric)
            assert np.array_equal(i1, i2) and np.array_equal(s1, s2) and np.array_equal(qp[0], keep), metric
            bi1, bs1 = ranking.rank_batch(h, qp, top_k=20, metric=metric)
            bi2, bs2 = ranking.rank_batch(h, qf.copy(), top_k=20, metric=metric)
            assert np.array_equal(bi1, bi2) and np.array_equal(bs1, bs2), metric
        ham = np.asarray(ranking.hamming_distance(h, qp[1]))
        assert np.array_equal(ham.astype(np.int64), d - (B != qb[1]).sum(axis=1))
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 10. refusals on the device path
# ------------------------------------------------------------------------------------------------
def test_no_shadow_and_no_row_list(pair):
    import torch
    from hyperdb._native import METRIC_IDS
    b1, i8, _ = pair
    with pytest.raises(NotImplementedError):
        b1.quantize("int8")
    assert b1.stat("quant_bytes") == 0
    rng = np.random.default_rng(10)
    rows = np.sort(rng.choice(N, size=N // 64, replace=False)).astype(np.int64)
    mask = np.zeros(N, dtype=np.uint8)
    mask[rows] = 1
    Q = _queries(384)[:4]
    try:
        for ix in (b1, i8):
            ix.set_option("subset_min_n", 0)
        for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "manhattan_distance", "pearson_correlation"):
            for nq in (1, 4):
                mid = METRIC_IDS[metric]
                b1.set_row_mask(mask)
                wi, ws, wst = b1.topk_device(Q[:nq], 30, mid)
                b1.set_row_subset(mask, rows)
                gi, gs, gst = b1.topk_device(Q[:nq], 30, mid)
                assert b1.stat("subset") == 0 and b1.stat("subset_rows") == rows.size, (metric, nq)
                assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), (metric, nq)
                assert mask[gi.cpu().numpy()].all()
                i8.set_row_subset(mask, rows)
                i8.topk_device(Q[:nq], 30, mid)
                assert i8.stat("subset") == 1, (metric, nq)       # (the list is eligible: an int8 index over the same values takes it)
    finally:
        for ix in (b1, i8):
            ix.set_row_mask(None)
            ix.set_option("subset_min_n", -1)
