"""GPU tests (-m gpu) of packed-bit batches on the bf16 matrix cores (csrc/hdb_mfma_b1.h), the opt-in set_option("b1_mfma_min_q", n).

The contract: a bit is exactly one bf16 number and the kernel walks K as the bfloat16 flavour does, so with the option on a packed-bit
index returns, for dot / cosine / euclidean batches of 5+ queries, the indices, float32 score bits and status words of a
torch.bfloat16 index over the unpacked 0/1 matrix on the same device -- whole rows of 128 .. 512 elements and the K slices of wider
ones.  Pearson goes through the cosine epilogue with a row scale of its own bits: oracle/ranking_oracle.py (float64) at the project's
float32 contract 1e-5 * max(1, |s|), and the default path's index set modulo ties inside it.  Everything else -- manhattan, the
bit metrics, 1-4 queries, other widths, use_mfma = 0, and every call without the option -- stays on the bit scan with its bits.

Shapes: n = 20 003 (ragged last tile, the sampled pipeline), density 0.5 with one all-zero and one all-one row."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 20_003
MM_METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")


@pytest.fixture(scope="module")
def orc():
    from oracle import ranking_oracle
    return ranking_oracle


_MATS = {}


def _matrix(d, n=N):
    """(bool bits [n, d], their float32 0/1 widening) per shape, shared by the tests and never modified."""
    if (d, n) not in _MATS:
        rng = np.random.default_rng(4000 * d + n)
        B = rng.random((n, d)) < 0.5
        B[7] = False                                     # an all-zero row and an all-one row
        B[n - 5] = True
        _MATS[(d, n)] = (B, B.astype(np.float32))
    return _MATS[(d, n)]


@pytest.fixture(scope="module")
def pairs():
    """d -> (packed-bit index with the option on, bfloat16 index over the unpacked matrix, host widening), built once."""
    import torch
    from hyperdb._native import GpuIndex
    made = {}

    def get(d):
        if d not in made:
            B, Bw = _matrix(d)
            b1 = GpuIndex(np.packbits(B, axis=1), storage="bits")
            bf = GpuIndex(torch.from_numpy(Bw).to(torch.bfloat16).cuda())
            assert b1.dtype == 10 and bf.dtype == 3
            b1.set_option("b1_mfma_min_q", 5)
            assert b1.stat("b1_mfma_min_q") == 5
            bf.set_option("bf16_ks_min_q", 5)            # (the slices of a wide bf16 row from the same batch sizes on)
            made[d] = (b1, bf, Bw)
        return made[d]

    yield get
    for b1, bf, _ in made.values():
        b1.close()
        bf.close()


def _same_bits(b1, bf, Q, k, mid, exact, tag):
    gi, gs, gst = b1.topk_device(Q, k, mid, exact=exact)
    assert b1.stat("mfma") == 1 and b1.stat("fused") == 0 and b1.stat("quant") == 0 and b1.stat("path") == (2 if exact else 1), tag
    wi, ws, wst = bf.topk_device(Q, k, mid, exact=exact)
    assert bf.stat("mfma") == 1, tag
    gi, gs, gst, wi, ws, wst = (t.cpu().numpy() for t in (gi, gs, gst, wi, ws, wst))
    assert np.array_equal(gi, wi), tag
    assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), tag
    assert np.array_equal(gst, wst), tag
    return gi, gs


def _bit_contract(orc, pairs, d, nq, oracle_queries):
    from hyperdb._native import METRIC_IDS
    b1, bf, Bw = pairs(d)
    rng = np.random.default_rng(31 * d + nq)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[0] = Bw[N - 2]                                     # a stored row of the ragged last tile, as 0/1 floats
    bias = rng.uniform(-0.5, 0.5, N).astype(np.float32)
    mask = (rng.random(N) < 0.02).astype(np.uint8)
    mask[:3] = 1
    k = 50
    try:
        for metric in MM_METRICS:
            mid = METRIC_IDS[metric]
            gi, gs = _same_bits(b1, bf, Q, k, mid, False, (d, nq, metric, "plain"))
            for qi in oracle_queries:                    # ... and the answer itself, against the oracle
                orc.check_topk(gi[qi], gs[qi], Bw, Q[qi], metric, k, tol=TOL)
            if metric == "euclidean_metric":
                assert gi[0][0] == N - 2 and gs[0][0] == 1.0
            _same_bits(b1, bf, Q, k, mid, True, (d, nq, metric, "exact"))
            for ix in (b1, bf):
                ix.set_bias(bias)
            bi, bs = _same_bits(b1, bf, Q, k, mid, False, (d, nq, metric, "bias"))
            if oracle_queries:
                orc.check_topk(bi[1], bs[1], Bw, Q[1], metric, k, bias=bias.astype(np.float64), tol=TOL)
            for ix in (b1, bf):
                ix.set_bias(None)
                ix.set_row_mask(mask)
            mi, _ = _same_bits(b1, bf, Q, k, mid, False, (d, nq, metric, "mask"))
            assert mask[mi].all()
            for ix in (b1, bf):
                ix.set_row_mask(None)
    finally:
        for ix in (b1, bf):
            ix.set_bias(None)
            ix.set_row_mask(None)


@pytest.mark.parametrize("nq", [5, 16, 17, 64])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_bits_of_a_bfloat16_index(orc, pairs, d, nq):
    _bit_contract(orc, pairs, d, nq, sorted({0, nq // 2, nq - 1}))


@pytest.mark.parametrize("nq", [5, 17])
@pytest.mark.parametrize("d", [640, 768, 1024, 4096])
def test_slices_bits_of_a_bfloat16_index(orc, pairs, d, nq):
    _bit_contract(orc, pairs, d, nq, (0, nq - 1) if d <= 1024 else ())      # (the float64 oracle over 20 003 x 4096 is left to the narrower rows)


@pytest.mark.parametrize("d", [384, 768])
def test_pearson(orc, pairs, d):
    """The row scale 1 / (sd_v d) comes from a closed form in float64 and need not have the bits of the bf16 index's scale: the
    oracle at the float32 tolerance, and the default path's index set modulo ties inside it."""
    from hyperdb._native import METRIC_IDS
    b1, _, Bw = pairs(d)
    mid = METRIC_IDS["pearson_correlation"]
    Q = np.random.default_rng(5 + d).standard_normal((16, d)).astype(np.float32)
    k = 50
    try:
        gi, gs, gst = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid))
        assert b1.stat("mfma") == 1 and b1.stat("path") == 1 and (gst == 0).all()
        b1.set_option("b1_mfma_min_q", 0)
        wi, ws, wst = (t.cpu().numpy() for t in b1.topk_device(Q, k, mid))
        assert b1.stat("mfma") == 0 and (wst == 0).all()
        for qi in range(16):
            assert orc.same_result_modulo_ties(gi[qi], gs[qi], wi[qi], ws[qi], TOL), qi
        for qi in (0, 7, 15):
            orc.check_topk(gi[qi], gs[qi], Bw, Q[qi], "pearson_correlation", k, tol=TOL)
    finally:
        b1.set_option("b1_mfma_min_q", 5)


@pytest.mark.parametrize("at", [0, N - 128])
def test_every_bit_position(at):
    """Rows at .. at + 127 one-hot (row at + i holds bit i), every other row all-zero; 16 queries, each a permutation of 128 distinct
    positive values with all three bf16 parts in use: the dot product of row at + i is query element i exactly, so the answer is the
    50 largest query elements at their own rows."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    B = np.zeros((N, 128), dtype=bool)
    B[at + np.arange(128), np.arange(128)] = True
    rng = np.random.default_rng(at + 1)
    vals = (np.arange(1, 129) / 7.0).astype(np.float32)
    assert np.unique(vals).size == 128 and (vals > 0).all()
    Q = np.stack([rng.permutation(vals) for _ in range(16)]).astype(np.float32)
    ix = GpuIndex(np.packbits(B, axis=1), storage="bits")
    try:
        ix.set_option("b1_mfma_min_q", 5)
        gi, gs, gst = (t.cpu().numpy() for t in ix.topk_device(Q, 50, METRIC_IDS["dot_product"], exact=True))
        assert ix.stat("mfma") == 1 and ix.stat("path") == 2 and (gst == 0).all()
        for qi in range(16):
            order = np.argsort(-Q[qi], kind="stable")[:50]
            assert np.array_equal(gi[qi], at + order), qi
            assert np.array_equal(gs[qi].view(np.uint32), Q[qi][order].view(np.uint32)), qi
    finally:
        ix.close()


def test_what_stays_on_the_bit_scan(pairs):
    """With the option on, manhattan, the bit metrics, 1-4 queries, a width without a kernel and use_mfma = 0 keep the bit scan: the
    bits of the same call with the option off."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    b1, _, _ = pairs(384)
    B544 = _matrix(544)[0]
    odd = GpuIndex(np.packbits(B544, axis=1), storage="bits")
    Q = np.random.default_rng(3).standard_normal((16, 384)).astype(np.float32)
    Q544 = np.random.default_rng(4).standard_normal((16, 544)).astype(np.float32)
    cos = "cosine_similarity"
    cases = [(b1, Q, "manhattan_distance", {}), (b1, Q, "hamming_distance", {}), (b1, Q, "jaccard_similarity", {}),
             (b1, Q[:1], cos, {}), (b1, Q[:4], cos, {}), (b1, Q[:4], "euclidean_metric", {}), (odd, Q544, cos, {}),
             (b1, Q, cos, {"use_mfma": 0}), (b1, Q, "dot_product", {"use_mfma": 0})]
    try:
        odd.set_option("b1_mfma_min_q", 5)
        assert odd.stat("b1_mfma_min_q") == 0            # (no kernel for the width: never)
        for ix, q, metric, opts in cases:
            mid = METRIC_IDS[metric]
            for name, value in opts.items():
                ix.set_option(name, value)
            ix.set_option("b1_mfma_min_q", 5)
            gi, gs, gst = ix.topk_device(q, 50, mid)
            assert ix.stat("mfma") == 0, (metric, q.shape, opts)
            ix.set_option("b1_mfma_min_q", 0)
            wi, ws, wst = ix.topk_device(q, 50, mid)
            assert ix.stat("mfma") == 0
            assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), (metric, q.shape, opts)
            for name in opts:
                ix.set_option(name, 1)
            ix.set_option("b1_mfma_min_q", 5)
    finally:
        b1.set_option("use_mfma", 1)
        b1.set_option("b1_mfma_min_q", 5)
        odd.close()


def test_default_is_the_bit_scan():
    from hyperdb._native import GpuIndex, METRIC_IDS
    ix = GpuIndex(np.packbits(_matrix(384)[0], axis=1), storage="bits")
    try:
        assert ix.stat("b1_mfma_min_q") == 0
        Q = np.random.default_rng(6).standard_normal((16, 384)).astype(np.float32)
        for metric in MM_METRICS:
            ix.topk_device(Q, 50, METRIC_IDS[metric])
            assert ix.stat("mfma") == 0 and ix.stat("path") == 1, metric
        ix.set_option("b1_mfma_min_q", -1)               # the measured rule of the width, never below 5; 0 = never
        assert ix.stat("b1_mfma_min_q") == 0 or ix.stat("b1_mfma_min_q") >= 5
        ix.set_option("b1_mfma_min_q", 3)
        assert ix.stat("b1_mfma_min_q") == 5
        ix.set_option("b1_mfma_min_q", 16)
        assert ix.stat("b1_mfma_min_q") == 16
        ix.topk_device(Q[:15], 50, METRIC_IDS["cosine_similarity"])
        assert ix.stat("mfma") == 0
        ix.topk_device(Q, 50, METRIC_IDS["cosine_similarity"])
        assert ix.stat("mfma") == 1
    finally:
        ix.close()


def test_lifecycle_with_the_option_on():
    """append / update / compact with the option on: a 16-query cosine call equals a fresh index over the resulting rows, bit for bit."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 256
    rng = np.random.default_rng(8)
    rows = rng.random((24_000, d)) < 0.5
    pk = lambda b: np.packbits(b, axis=1)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    mid = METRIC_IDS["cosine_similarity"]

    def same_as_fresh(ix, now, tag):
        assert ix.n == now.shape[0], tag
        fresh = GpuIndex(pk(now), storage="bits")
        try:
            fresh.set_option("b1_mfma_min_q", 5)
            gi, gs, gst = ix.topk_device(Q, 40, mid)
            assert ix.stat("mfma") == 1, tag
            wi, ws, wst = fresh.topk_device(Q, 40, mid)
            assert fresh.stat("mfma") == 1, tag
            assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), tag
        finally:
            fresh.close()

    ix = GpuIndex(pk(rows[:9_000]), storage="bits")
    try:
        ix.set_option("b1_mfma_min_q", 5)
        ix.topk_device(Q, 40, mid)                        # the row norms exist before the matrix grows
        ix.append(pk(rows[9_000:12_001]))                 # the allocation grows (rebase); a ragged last tile
        same_as_fresh(ix, rows[:12_001], "append")
        keep = np.sort(rng.choice(12_001, size=10_007, replace=False))
        ix.compact(keep)
        same_as_fresh(ix, rows[:12_001][keep], "compact")
        ix.update(pk(rows[12_001:24_000]))
        same_as_fresh(ix, rows[12_001:24_000], "update")
    finally:
        ix.close()


@pytest.mark.parametrize("d", [384, 640])
def test_base_aligned_to_four_bytes_only(d):
    """hdb_index_create guarantees a packed matrix 4-byte alignment only.  The shim hands a bitorder="little" device tensor over
    without a copy, so a view that starts 4 bytes into a buffer is such a base: the call succeeds with the answers of an aligned copy."""
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    B = _matrix(d)[0]
    packed = torch.from_numpy(np.packbits(B, axis=1, bitorder="little")).cuda()
    cols = d // 8
    buf = torch.zeros(N * cols + 64, dtype=torch.uint8, device="cuda")
    view = buf[4:4 + N * cols].view(N, cols)
    view.copy_(packed)
    assert view.data_ptr() % 8 == 4 and packed.data_ptr() % 16 == 0
    odd = GpuIndex(view, storage="bits", bitorder="little")
    even = GpuIndex(packed, storage="bits", bitorder="little")
    try:
        assert odd.V.data_ptr() == view.data_ptr(), "the shim copied the view: this case needs a device tensor handed over as it is"
        Q = np.random.default_rng(9 + d).standard_normal((17, d)).astype(np.float32)
        for ix in (odd, even):
            ix.set_option("b1_mfma_min_q", 5)
        for metric in MM_METRICS:
            for exact in (False, True):
                gi, gs, gst = odd.topk_device(Q, 50, METRIC_IDS[metric], exact=exact)
                assert odd.stat("mfma") == 1, (metric, exact)
                wi, ws, wst = even.topk_device(Q, 50, METRIC_IDS[metric], exact=exact)
                assert even.stat("mfma") == 1, (metric, exact)
                assert torch.equal(gi, wi) and torch.equal(gs.view(torch.int32), ws.view(torch.int32)) and torch.equal(gst, wst), (metric, exact)
    finally:
        odd.close()
        even.close()


# every packed-bit shard launcher of the matrix-core scan x {dot, cosine, euclidean} x {no bias, bias} (tests/launcher_cells.py;
# profiles/mfma_launch_coverage.txt): whole rows and K slices (d = 640: slices of 384 / 256, d = 1024: of 512); 5 queries and 17,
# where the register kernel's query groups per workgroup go from one to two
@pytest.mark.parametrize("d,nq", [(128, 5), (128, 17), (256, 5), (384, 5), (512, 5), (512, 17), (640, 5), (640, 17), (1024, 5)])
def test_every_b1_launcher_metric_and_bias(orc, d, nq):
    import launcher_cells
    launcher_cells.check_launcher_cells(orc, "b1", d, nq, {"b1_mfma_min_q": 5}, TOL, {"mfma": 1, "fused": 0})
