"""GPU tests (-m gpu) of int8 storage (storage="int8", HDB_I8 = 7): an np.int8 / torch.int8 matrix stays one byte per element on the
device, the VALU scans serve every metric on it, and batches of 5+ dot / cosine / euclidean / pearson queries run on the bf16
matrix cores (hdb_mfma_i8.hip: the float8 kernel with the int8 row converter).

References.  VALU paths: oracle/ranking_oracle.py on the float32 widening of the matrix -- every stored integer IS a float32 value
and every path computes in float32 on it, so the tolerance is the project's float32 contract, 1e-5 applied as tol * max(1, |s|);
hamming is exact (sign bit x > 0), jaccard 1e-6.  Matrix cores: a torch.bfloat16 index over V.to(torch.bfloat16) on the same
device -- the conversion is exact (|x| <= 128 has 8 significant bits) and the K walk and epilogue are shared, so indices, float32
score BITS and status words must be equal.

Full score vectors over all rows are compared for cosine and pearson (and the integer-valued bit metrics); dot, euclidean and
manhattan are checked on the top-k rows and by the one-hot test: with full-range codes two float32 summation orders of one row
differ by up to 1.5e-3 (checked on a CPU, d = 100 / 384 / 512), so a row with |s| < 100 breaks 1e-5 * max(1, |s|) between two
CORRECT float32 results, while the top-100 rows (|s| >= 2 000) and all cosine scores showed no violation.
Matrices come from rng.integers(-128, 128)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric", "hamming_distance", "manhattan_distance",
           "jaccard_similarity", "pearson_correlation")
FULL_VECTOR = ("cosine_similarity", "pearson_correlation", "hamming_distance", "jaccard_similarity")
MM_METRICS = ("cosine_similarity", "dot_product", "euclidean_metric", "pearson_correlation")
N = 20_003                                             # many tiles per workgroup, ragged last 16-row tile


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


_MATS = {}


def _matrix(d, n=N):
    """One (int8 host array, its float32 widening) per shape, shared by the tests and never modified."""
    key = (d, n)
    if key not in _MATS:
        rng = np.random.default_rng(1000 * d + n)
        V = rng.integers(-128, 128, size=(n, d)).astype(np.int8)
        _MATS[key] = (V, V.astype(np.float32))
    return _MATS[key]


def _all_codes(rows, cols):
    """rows x cols int8 with every one of the 256 codes present, at random places."""
    rng = np.random.default_rng(rows + cols)
    codes = rng.integers(-128, 128, size=(rows, cols)).astype(np.int8)
    codes.reshape(-1)[rng.permutation(codes.size)[:256]] = np.arange(-128, 128).astype(np.int8)
    assert len(set(codes.reshape(-1).tolist())) == 256
    return codes


# ------------------------------------------------------------------------------------------------
# 1. storage and codes
# ------------------------------------------------------------------------------------------------
def test_storage_is_one_byte_per_element(ranking):
    import torch
    from hyperdb._native import GpuIndex, HDB_I8
    V, Vw = _matrix(100)
    for src in (V, torch.from_numpy(V), torch.from_numpy(V).cuda(), Vw, V.astype(np.int64)):
        ix = GpuIndex(src, storage="int8")
        try:
            assert ix.dtype == HDB_I8 == 7 and ix.storage == "int8"
            assert ix.V.dtype == torch.int8 and ix.V.element_size() * ix.n * ix.d == N * 100
            host = ix.host_matrix()
            assert host.dtype == np.float32 and np.array_equal(host, Vw)
            assert not ix.has_nan
        finally:
            ix.close()
    with pytest.raises(ValueError, match=r"\.5"):
        GpuIndex(Vw[:10] + 0.5, storage="int8")
    # without the keyword an int8 tensor is still a float64 index and a raw tensor handed to a metric function answers in float64
    ix = GpuIndex(torch.from_numpy(V[:300]))
    try:
        assert ix.dtype == 2 and ix.V.dtype == torch.float64
    finally:
        ix.close()
    q = np.ones(100, dtype=np.float32)
    assert np.asarray(ranking.dot_product(torch.from_numpy(V[:300]), q)).dtype == np.float64
    h = ranking.register_vectors(V[:300], storage="int8")
    try:
        got = np.asarray(ranking.dot_product(h, q))
        assert got.dtype == np.float32 and np.array_equal(got, Vw[:300].sum(axis=1))      # (integer sums below 2^24: exact)
        got = np.asarray(ranking.dot_product(h.index, q))
        assert got.dtype == np.float32
    finally:
        h.close()


def test_every_code_at_every_byte_position(ranking):
    """One-hot queries: the dot product with e_j is column j of the matrix, exactly -- pins the byte order of all 16 positions of a
    chunk and the widening of every code; 48 bytes through the runtime loop (three chunks, the lanes past the third idle), 384
    bytes through the unrolled kernel."""
    for cols, picks in ((48, range(48)), (384, (0, 1, 2, 3, 15, 16, 17, 63, 100, 127, 128, 255, 256, 300, 382, 383))):
        codes = _all_codes(1024, cols)
        wide = codes.astype(np.float32)
        h = ranking.register_vectors(codes, storage="int8")
        try:
            assert not h.index.has_nan
            for j in picks:
                q = np.zeros(cols, dtype=np.float32)
                q[j] = 1.0
                got = np.asarray(ranking.dot_product(h, q))
                assert got.dtype == np.float32 and got.shape == (1024,) and np.array_equal(got, wide[:, j]), (cols, j)
        finally:
            h.close()


# ------------------------------------------------------------------------------------------------
# 2. VALU scans: every metric at d = 384 / 256 / 512 (the unrolled kernels of 24 / 16 / 32 chunks), 272 (17 chunks: the generic
#    vector kernel) and 100 (the element-wise scan); 1 and 4 queries, k = 100
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [384, 256, 512, 272, 100])
def test_valu_scans_all_metrics(ranking, orc, d):
    V, Vw = _matrix(d)
    rng = np.random.default_rng(d)
    Q = rng.standard_normal((4, d)).astype(np.float32)
    Q[1] = Vw[N - 2] + 3.0 * rng.standard_normal(d).astype(np.float32)       # near a row of the ragged last tile
    k = 100
    h = ranking.register_vectors(V, storage="int8")
    try:
        for metric in METRICS:
            tol = _tol(metric)
            oracle = [orc.rank(Vw, Q[qi].copy(), top_k=k, metric=metric) for qi in range(4)]
            idx, sc = ranking.hyperDB_ranking_algorithm_sort(h, Q[0].copy(), top_k=k, metric=metric)
            assert h.index.stat("mfma") == 0
            orc.check_topk(idx, sc, Vw, Q[0], metric, k, tol=tol)
            assert orc.same_result_modulo_ties(idx, sc, oracle[0][0], oracle[0][1], tol), metric
            bi, bs = ranking.rank_batch(h, Q.copy(), top_k=k, metric=metric)
            assert h.index.stat("mfma") == 0
            for qi in range(4):
                orc.check_topk(bi[qi], bs[qi], Vw, Q[qi], metric, k, tol=tol)
                assert orc.same_result_modulo_ties(bi[qi], bs[qi], oracle[qi][0], oracle[qi][1], tol), (metric, qi)
            if metric in FULL_VECTOR:                    # the per-metric function: all N scores
                got = getattr(ranking, metric)(h, Q[1].copy()).astype(np.float64)
                want = orc.exact_scores(Vw, Q[1], metric)
                assert got.shape == (N,)
                if metric == "hamming_distance":
                    assert np.array_equal(got, want)
                else:
                    err = np.abs(got - want)
                    print(f"d={d} {metric}: largest score error {err.max():.3e}")
                    assert np.all(err <= tol * np.maximum(1.0, np.abs(want))), (metric, err.max())
    finally:
        h.close()


# ------------------------------------------------------------------------------------------------
# 3. matrix-core batches: the bits of a bfloat16 index over the same values
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs():
    """d -> (int8 index, bfloat16 index over the same values, host widening) at 20 003 x d, built once and closed with the module."""
    import torch
    from hyperdb._native import GpuIndex
    made = {}

    def get(d):
        if d not in made:
            V, Vw = _matrix(d)
            i8 = GpuIndex(V, storage="int8")
            bf = GpuIndex(torch.from_numpy(V).to(torch.bfloat16).cuda())
            assert i8.dtype == 7 and bf.dtype == 3 and np.array_equal(bf.host_matrix(), Vw) and np.array_equal(i8.host_matrix(), Vw)
            made[d] = (i8, bf, Vw)
        return made[d]

    yield get
    for i8, bf, _ in made.values():
        i8.close()
        bf.close()


def _same_bits(i8, bf, Q, k, mid, exact, tag):
    gi, gs, gst = i8.topk_device(Q, k, mid, exact=exact)
    assert i8.stat("mfma") == 1 and i8.stat("fused") == 0 and i8.stat("quant") == 0 and i8.stat("path") == (2 if exact else 1), tag
    wi, ws, wst = bf.topk_device(Q, k, mid, exact=exact)
    assert bf.stat("mfma") == 1, tag
    gi, gs, gst, wi, ws, wst = (t.cpu().numpy() for t in (gi, gs, gst, wi, ws, wst))
    assert np.array_equal(gi, wi), tag
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), tag
    assert np.array_equal(gst, wst), tag
    return gi, gs


@pytest.mark.parametrize("nq", [5, 16, 17, 64])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_matrix_core_bits_equal_a_bfloat16_index(orc, pairs, d, nq):
    from hyperdb._native import METRIC_IDS
    i8, bf, Vw = pairs(d)
    rng = np.random.default_rng(31 * d + nq)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[0] = Vw[N - 2]                                     # exact duplicate of a row in the ragged last tile (euclidean: re-scored)
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    mask = (rng.random(N) < 0.02).astype(np.uint8)
    mask[:3] = 1
    k = 50
    try:
        for metric in MM_METRICS:
            mid = METRIC_IDS[metric]
            gi, gs = _same_bits(i8, bf, Q, k, mid, False, (d, nq, metric, "plain"))
            for qi in sorted({0, nq // 2, nq - 1}):       # ... and the answer itself, against the oracle
                orc.check_topk(gi[qi], gs[qi], Vw, Q[qi], metric, k, tol=TOL)
            if metric == "euclidean_metric":
                assert gi[0][0] == N - 2 and gs[0][0] == 1.0
            _same_bits(i8, bf, Q, k, mid, True, (d, nq, metric, "exact"))
            for ix in (i8, bf):
                ix.set_bias(bias)
            bi, bs = _same_bits(i8, bf, Q, k, mid, False, (d, nq, metric, "bias"))
            orc.check_topk(bi[1], bs[1], Vw, Q[1], metric, k, bias=bias.astype(np.float64), tol=TOL)
            for ix in (i8, bf):
                ix.set_bias(None)
                ix.set_row_mask(mask)
            mi, _ = _same_bits(i8, bf, Q, k, mid, False, (d, nq, metric, "mask"))
            assert mask[mi].all()
            for ix in (i8, bf):
                ix.set_row_mask(None)
    finally:
        for ix in (i8, bf):
            ix.set_bias(None)
            ix.set_row_mask(None)


def test_matrix_core_all_codes():
    """The all-codes matrix tiled to 20 003 x 128: every code meets the row converter at every byte position of a fragment."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    V = np.resize(_all_codes(1024, 48), (N, 128)).copy()
    for j in range(8):                                   # ... and every code at each of the eight byte positions a lane converts
        V[2_000 + 256 * j:2_000 + 256 * (j + 1), j + 8 * (2 * j + 1)] = np.arange(-128, 128).astype(np.int8)
    assert len(set(V.reshape(-1).tolist())) == 256
    for j in range(8):
        assert len(set(V[:, j::8].reshape(-1).tolist())) == 256, j
    Q = np.random.default_rng(128).standard_normal((16, 128)).astype(np.float32)
    Q[:8] = np.eye(128, dtype=np.float32)[[0, 1, 2, 3, 4, 5, 6, 7]]
    i8 = GpuIndex(V, storage="int8")
    bf = GpuIndex(torch.from_numpy(V).to(torch.bfloat16).cuda())
    try:
        for metric in MM_METRICS:
            gi, gs = _same_bits(i8, bf, Q, 50, METRIC_IDS[metric], False, ("codes", metric))
            if metric == "dot_product":
                for j in range(8):                       # one-hot queries: the 50 largest entries of column j, exactly
                    col = V[:, j].astype(np.float32)
                    assert np.array_equal(gs[j], np.sort(col)[::-1][:50]) and np.array_equal(col[gi[j]], gs[j]), j
    finally:
        i8.close()
        bf.close()


# ------------------------------------------------------------------------------------------------
# 4. the rest: full sort, row list, lifecycle, no shadow, group, facade
# ------------------------------------------------------------------------------------------------
def test_full_sort(orc):
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Vw = _matrix(384)
    Q = np.random.default_rng(3).standard_normal((2, 384)).astype(np.float32)
    ix = GpuIndex(V, storage="int8")
    try:
        k = 3_000
        for metric in ("cosine_similarity", "euclidean_metric"):
            fi, fs = ix.topk(Q, k, METRIC_IDS[metric])
            assert ix.stat("path") == 3
            for qi in range(2):
                orc.check_topk(fi[qi], fs[qi], Vw, Q[qi], metric, k, tol=TOL)
    finally:
        ix.close()


def test_row_list_equals_a_fresh_index():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    n, d, k = 70_001, 384, 30
    V, _ = _matrix(d, n)
    rng = np.random.default_rng(64)
    rows = np.sort(rng.choice(n, size=n // 64, replace=False)).astype(np.int64)
    mask = np.zeros(n, dtype=np.uint8)
    mask[rows] = 1
    Q = rng.standard_normal((4, d)).astype(np.float32)
    ix = GpuIndex(V, storage="int8")
    fresh = GpuIndex(V[rows], storage="int8")
    try:
        ix.set_row_subset(mask, rows)
        for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "manhattan_distance", "pearson_correlation"):
            for nq in (1, 4):
                gi, gs, gst = ix.topk_device(Q[:nq], k, METRIC_IDS[metric])
                assert ix.stat("subset") == 1 and ix.stat("subset_rows") == rows.size and ix.stat("mfma") == 0 and ix.stat("fused") == 0
                wi, ws, wst = fresh.topk_device(Q[:nq], k, METRIC_IDS[metric])
                tag = (metric, nq)
                assert np.array_equal(gi.cpu().numpy(), rows[wi.cpu().numpy()]), tag
                assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), tag
    finally:
        ix.close()
        fresh.close()


def test_append_compact_update_and_no_shadow():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 128
    V, Vw = _matrix(d)
    rng = np.random.default_rng(12)
    extra = rng.integers(-128, 128, size=(3_001, d)).astype(np.int8)
    extra_w = extra.astype(np.float32)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    n0 = 9_000
    ix = GpuIndex(V[:n0], storage="int8")
    try:
        ix.topk(Q[:1], 5, METRIC_IDS["hamming_distance"])                  # builds the sign-bit cache that append must extend
        ix.append(extra_w[:1])                                             # integer float data: converted on the way in
        assert ix.n == n0 + 1 and np.array_equal(ix.host_matrix()[n0:], extra_w[:1])
        with pytest.raises(ValueError, match=r"\.5"):
            ix.append(extra_w[1:3] + 0.5)
        with pytest.raises(ValueError, match="128"):
            ix.append(np.full((1, d), 128, dtype=np.int64))
        assert ix.n == n0 + 1                                              # nothing of a refused call is stored
        ix.append(extra[1:2000])                                           # int8 as it is
        ix.append(torch.from_numpy(extra[2000:]).cuda())                   # ... from the device too
        assert ix.n == n0 + 3_001 and ix.V.dtype == torch.int8 and ix.V.element_size() == 1
        assert np.array_equal(ix.host_matrix()[n0:], extra_w) and np.array_equal(ix.host_matrix()[:n0], Vw[:n0])
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        ix.compact(keep)
        assert ix.n == keep.size and ix.V.dtype == torch.int8
        fresh = GpuIndex(np.concatenate([V[:n0], extra])[keep], storage="int8")
        try:
            assert np.array_equal(ix.host_matrix(), fresh.host_matrix())
            for metric in ("cosine_similarity", "euclidean_metric", "dot_product", "hamming_distance", "pearson_correlation"):
                for sl in (slice(0, 1), slice(0, 16)):
                    i1, s1 = ix.topk(Q[sl], 30, METRIC_IDS[metric])
                    m1 = ix.stat("mfma")
                    i2, s2 = fresh.topk(Q[sl], 30, METRIC_IDS[metric])
                    assert m1 == fresh.stat("mfma") == (1 if (sl.stop == 16 and metric != "hamming_distance") else 0), (metric, sl)
                    assert np.array_equal(i1, i2) and np.array_equal(s1, s2), (metric, sl)
        finally:
            fresh.close()
        with pytest.raises(NotImplementedError, match="int8"):
            ix.quantize("int8")
        ix.set_option("quant_min_n", 0)
        ix.topk(Q[:1], 30, METRIC_IDS["cosine_similarity"])
        assert ix.stat("quant_auto") == 0 and ix.stat("quant") == 0
        # update: integer float data into an int8 index is converted the same way; anything else is refused and nothing changes
        ix.update(torch.from_numpy(extra_w).cuda())
        assert ix.n == 3_001 and ix.V.dtype == torch.int8 and np.array_equal(ix.host_matrix(), extra_w)
        with pytest.raises(ValueError, match=r"\.5"):
            ix.update(extra_w[:50] + 0.5)
        assert ix.n == 3_001
        ix.update(extra[:100])
        assert ix.n == 100 and np.array_equal(ix.host_matrix(), extra_w[:100])
    finally:
        ix.close()


def test_two_shards_on_one_device(ranking):
    """register_vectors(..., devices=[0, 0], storage="int8"): the merged answer is the single index's."""
    import torch
    V, Vw = _matrix(384)
    Q = np.random.default_rng(31).standard_normal((5, 384)).astype(np.float32)
    one = ranking.register_vectors(V, storage="int8")
    two = ranking.register_vectors(Vw, devices=[0, 0], storage="int8")     # (integer float data: converted before the split)
    try:
        assert all(s.V.dtype == torch.int8 and s.dtype == 7 for s in two.index.shards) and len(two.index.shards) == 2
        assert np.array_equal(two.index.host_matrix(), Vw)
        for metric in ("cosine_similarity", "euclidean_metric", "hamming_distance"):
            a = ranking.rank_batch(one, Q.copy(), top_k=15, metric=metric)
            b = ranking.rank_batch(two, Q.copy(), top_k=15, metric=metric)
            assert np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1])), metric
        with pytest.raises(ValueError, match=r"\.[27]5"):
            ranking.register_vectors(Vw[:100] + 0.25, devices=[0, 0], storage="int8")
    finally:
        one.close()
        two.close()


def test_facade_int8(tmp_path, orc):
    import torch
    from hyperdb import HyperDB
    rng = np.random.default_rng(21)
    n, d = 9_001, 128
    V = rng.integers(-128, 128, size=(n, d)).astype(np.int8)
    Vw = V.astype(np.float32)
    docs = [{"id": i, "text": f"doc {i}"} for i in range(n)]
    Q = rng.standard_normal((8, d)).astype(np.float32)
    db = HyperDB([dict(x) for x in docs], V, storage="int8")
    assert db._index.V.dtype == torch.int8 and db._index.dtype == 7 and db._index.V.element_size() == 1
    assert db.vectors.dtype == np.float32 and np.array_equal(db.vectors, Vw)
    for metric in ("cosine_similarity", "euclidean_metric", "dot_product"):
        res = db.query(Q[0], top_k=10, metric=metric)
        orc.check_topk(np.array([r[2] for r in res]), np.array([r[1] for r in res]), Vw, Q[0], metric, 10, tol=TOL)
        oi, osc = orc.rank(Vw, Q[0].copy(), top_k=10, metric=metric)
        assert orc.same_result_modulo_ties(np.array([r[2] for r in res]), np.array([r[1] for r in res]), oi, osc, TOL), metric
        assert [r[0] for r in res] == [docs[r[2]] for r in res]
        for qi, got in enumerate(db.query_batch(Q, top_k=10, metric=metric)):
            orc.check_topk(np.array([r[2] for r in got]), np.array([r[1] for r in got]), Vw, Q[qi], metric, 10, tol=TOL)
    # add converts with the same function; a value that is no int8 integer is refused and nothing of the call is stored
    db.add([{"id": -1}], Vw[:1])
    assert db._index.V.dtype == torch.int8 and db.vectors.shape == (n + 1, d) and np.array_equal(db.vectors[-1], Vw[0])
    with pytest.raises(ValueError, match=r"\.5"):
        db.add([{"id": -2}], Vw[:1] + 0.5)
    assert db.size() == n + 1 and len(db.documents) == n + 1
    db.remove_document(3)
    assert db.size() == n and np.array_equal(db.vectors[3], Vw[4])
    path = str(tmp_path / "db.pickle")
    db.save(path, format="pickle")
    back = HyperDB(storage="int8")
    back.load(path, format="pickle")
    assert back._index.V.dtype == torch.int8 and back._index.dtype == 7
    assert back.vectors.dtype == np.float32 and np.array_equal(back.vectors, db.vectors)
    a, b = back.query(Q[1], top_k=10), db.query(Q[1], top_k=10)
    assert [r[2] for r in a] == [r[2] for r in b] and [float(r[1]) for r in a] == [float(r[1]) for r in b]


# both int8 shard launchers of the matrix-core scan x {dot, cosine, euclidean} x {no bias, bias} (tests/launcher_cells.py;
# profiles/mfma_launch_coverage.txt); 5 queries and 17, where the register kernel's query groups per workgroup go from one to two
@pytest.mark.parametrize("nq", [5, 17])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_every_i8_launcher_metric_and_bias(orc, d, nq):
    import launcher_cells
    launcher_cells.check_launcher_cells(orc, "i8", d, nq, {}, TOL, {"mfma": 1, "fused": 0})
