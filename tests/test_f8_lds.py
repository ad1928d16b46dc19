"""GPU tests (-m gpu) of float8 e4m3 batches on the bf16 matrix cores with the rows expanded to bf16 in LDS once per workgroup
(csrc/hdb_mfma_f8_lds.h, option f8_lds_min_q; 0 = never by default).

The LDS flavour keeps the register flavour's arithmetic: the same query parts, fragment map, K walk and epilogue, and the plan's
sample rows and thresholds do not change.  So the first reference is an IDENTITY: indices, score bits (compared as int32) and status
words equal the same call on the same index with f8_lds_min_q = 0, sampled and exact -- no tolerance.  The second, at d = 256 / 384
and through the K slices, is the bfloat16 index over the widened matrix, whose bits the float8 kernels return.  The third is
oracle/ranking_oracle.py on the exactly widened float32 matrix at the project's float32 contract, 1e-5 applied as tol * max(1, |s|),
for queries 0, 1, nq // 2 and nq - 1.

Every case sets f8_lds_min_q: before the option existed set_option raised, so every test here failed.

Shapes: N = 20 003 rows (above the 8192-row small path; a ragged last 16-row tile, a ragged last stage at every stage height), grids of 8
and 3 workgroups (many stages per workgroup, an uneven split), 5 / 17 / 64 / 65 / 130 / 257 queries (a partial query group, waves
without queries, a nearly empty second grid row, a one-query second chunk behind 256).  The float64 scores the oracle compares
against are computed once per width and metric for the checked queries and shared, unchanged.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5
N = 20_003
NQS = (5, 17, 64, 65, 130, 257)
CHECKED = sorted({qi for nq in NQS + (33,) for qi in (0, 1, nq // 2, nq - 1)})
METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")


@pytest.fixture(scope="module")
def orc():
    from oracle import ranking_oracle
    return ranking_oracle


def _dev(t8):
    import torch
    return t8.contiguous().view(torch.uint8).cuda().view(torch.float8_e4m3fn)


def _f8(a32):
    """float32 array -> (float8 CUDA tensor, its exact float32 widening on the host); no code of the tensor is NaN."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a32, dtype=np.float32)).to(torch.float8_e4m3fn)
    Vb = _dev(t)
    assert int(((Vb.view(torch.uint8) & 0x7F) == 0x7F).sum().item()) == 0, "a NaN code (0x7F / 0xFF) in the matrix"
    return Vb, t.float().numpy()


def _exact_many(Vw, Q, metric):
    """float64 scores [len(Q)][N] of `metric` on the stored values (oracle.exact_scores' arithmetic)."""
    Q64 = np.asarray(Q, dtype=np.float64)
    out = np.empty((Q64.shape[0], Vw.shape[0]), dtype=np.float64)
    qn2 = (Q64 * Q64).sum(axis=1)
    for lo in range(0, Vw.shape[0], 4096):
        V = Vw[lo:lo + 4096].astype(np.float64)
        dots = Q64 @ V.T
        vn2 = (V * V).sum(axis=1)
        if metric == "dot_product":
            s = dots
        elif metric == "cosine_similarity":
            vn, qn = np.sqrt(vn2), np.sqrt(qn2)
            vn[vn == 0] = 1.0
            qn[qn == 0] = 1.0
            s = dots / (vn[None, :] * qn[:, None])
        else:
            d2 = np.maximum(vn2[None, :] + qn2[:, None] - 2.0 * dots, 0.0)
            for qi, r in zip(*np.nonzero(d2 < 0.25 * qn2[:, None])):      # near a query: the direct difference, as the oracle forms it
                diff = V[r] - Q64[qi]
                d2[qi, r] = (diff * diff).sum()
            s = 1.0 / (1.0 + np.sqrt(d2))
        out[:, lo:lo + V.shape[0]] = s
    return out


_CASE = {}


def _case(d):
    """The data recipe of test_f8_wide's _case at width d: rows and queries N(0, 1) clipped to the float8 range (+-448), query 0 an
    exact duplicate of a row in the ragged last tile, no NaN code.  One width at a time is kept, shared by its cases, never modified."""
    if _CASE.get("d") != d:
        _CASE.clear()
        _CASE["d"] = d
        rng = np.random.default_rng(977 * d + 1)
        V32 = rng.standard_normal((N, d)).astype(np.float32)
        V32[1234] *= 0.05
        np.clip(V32, -448.0, 448.0, out=V32)
        Vb, Vw = _f8(V32)
        del V32
        Q = rng.standard_normal((257, d)).astype(np.float32)
        Q[0] = Vw[N - 2]
        Q[1] = Vw[77] + 0.05 * rng.standard_normal(d).astype(np.float32)
        ts = 1.7e9 + rng.uniform(0, 30 * 86400.0, size=N)
        exact = {m: dict(zip(CHECKED, _exact_many(Vw, Q[CHECKED], m))) for m in METRICS}
        _CASE["data"] = (Vb, Vw, Q, ts, exact)
    return _CASE["data"]


def _index(Vb, blocks=8, lds=5, ks=None):
    from hyperdb._native import GpuIndex
    ix = GpuIndex(Vb)
    ix.set_option("max_blocks", blocks)
    if ks is not None:
        ix.set_option("f8_ks_min_q", ks)
    if lds is not None:
        ix.set_option("f8_lds_min_q", lds)               # unknown before the LDS flavour existed: every test that sets it fails there
    return ix


def _same(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32)) and torch.equal(a[2], b[2])


def _both(ix, Q, k, mid, exact, tag):
    """The call with the LDS flavour and with the register flavour on the same index -> the LDS answer, after the identity check."""
    ix.set_option("f8_lds_min_q", 5)
    lds = ix.topk_device(Q, k, mid, exact=exact)
    assert ix.stat("f8_lds") == 1 and ix.stat("mfma") == 1 and ix.stat("fused") == 0 and ix.stat("path") == (2 if exact else 1), tag
    assert int(lds[2].abs().sum().item()) == 0, tag
    ix.set_option("f8_lds_min_q", 0)
    reg = ix.topk_device(Q, k, mid, exact=exact)
    assert ix.stat("f8_lds") == 0 and ix.stat("mfma") == 1, tag
    ix.set_option("f8_lds_min_q", 5)
    assert _same(lds, reg), tag
    return lds


# ------------------------------------------------------------------------------------------------
# 1. whole rows: identity with the register flavour, the bfloat16 index's bits, the oracle
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_whole_rows_equal_the_register_flavour(orc, d, nq):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    k = 50
    Vb, Vw, Qall, ts, exact = _case(d)
    Q = Qall[:nq]
    bf = None
    for blocks in (8, 3):
        ix = _index(Vb, blocks)
        if d in (256, 384) and blocks == 8:
            bf = GpuIndex(torch.from_numpy(Vw).to(torch.bfloat16).cuda())
            bf.set_option("max_blocks", 8)
        try:
            for metric in METRICS:
                mid = METRIC_IDS[metric]
                for bias in (False, True):
                    b = None
                    for h in (ix, bf):
                        if h is not None:
                            if bias:
                                h.set_recency(ts, 0.5)
                            else:
                                h.set_bias(None)
                    if bias:
                        b = 0.5 * np.exp(ts - ts.max())
                    tag = (d, nq, blocks, metric, bias)
                    got = _both(ix, Q, k, mid, False, tag)
                    gex = _both(ix, Q, k, mid, True, tag)
                    assert torch.equal(got[0], gex[0]) and torch.equal(got[1], gex[1]), tag
                    if bf is not None and blocks == 8:
                        for ex, mine in ((False, got), (True, gex)):
                            ref = bf.topk_device(Q, k, mid, exact=ex)
                            assert bf.stat("mfma") == 1, tag
                            assert _same(mine, ref), (tag, ex)
                    if blocks == 8:
                        mi_h, ms_h = got[0].cpu().numpy(), got[1].cpu().numpy()
                        for qi in (0, 1, nq // 2, nq - 1):
                            ref = exact[metric][qi] if b is None else exact[metric][qi] + b
                            err = np.abs(ms_h[qi].astype(np.float64) - ref[mi_h[qi]]) / np.maximum(1.0, np.abs(ref[mi_h[qi]]))
                            print(f"{tag} query {qi}: largest score error {err.max():.3e} of the band {TOL:g}")
                            orc.check_topk(mi_h[qi], ms_h[qi], Vw, Q[qi], metric, k, bias=b, tol=TOL, exact=ref)
                        if metric == "euclidean_metric" and not bias:
                            assert mi_h[0][0] == N - 2 and abs(ms_h[0][0] - 1.0) < 1e-6 and mi_h[1][0] == 77, tag
        finally:
            ix.close()
            if bf is not None and blocks == 8:
                bf.close()
                bf = None


def test_pearson_and_a_row_mask():
    from hyperdb._native import METRIC_IDS
    Vb, Vw, Qall, _, _ = _case(384)
    ix = _index(Vb)
    try:
        for exact in (False, True):
            _both(ix, Qall[:65], 40, METRIC_IDS["pearson_correlation"], exact, ("pearson", exact))
    finally:
        ix.close()
    Vb, Vw, Qall, _, _ = _case(256)
    mask = (np.random.default_rng(11).random(N) < 0.02).astype(np.uint8)
    mask[:3] = 1
    mask[N - 2] = 1
    ix = _index(Vb, 3)
    try:
        ix.set_row_mask(mask)
        for metric in ("cosine_similarity", "euclidean_metric"):
            for exact in (False, True):
                got = _both(ix, Qall[:64], 40, METRIC_IDS[metric], exact, ("mask", metric, exact))
                mi, ms = got[0].cpu().numpy(), got[1].cpu().numpy()
                assert mask[mi].all() and np.isfinite(ms).all()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 2. K slices: the slices with the LDS flavour off, and a bfloat16 index through its slices
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [33, 130])
@pytest.mark.parametrize("d", [640, 1280])
def test_k_slices_equal_the_register_slices_and_bfloat16(d, nq):
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    k = 50
    Vb, Vw, Qall, ts, _ = _case(d)
    Q = Qall[:nq]
    ix = _index(Vb, 8, ks=5)
    bf = GpuIndex(torch.from_numpy(Vw).to(torch.bfloat16).cuda())
    try:
        bf.set_option("max_blocks", 8)
        bf.set_option("bf16_ks_min_q", 5)
        for metric in METRICS:
            mid = METRIC_IDS[metric]
            for bias in (False, True):
                for h in (ix, bf):
                    if bias:
                        h.set_recency(ts, 0.5)
                    else:
                        h.set_bias(None)
                for exact in (False, True):
                    tag = (d, nq, metric, bias, exact)
                    got = _both(ix, Q, k, mid, exact, tag)
                    ref = bf.topk_device(Q, k, mid, exact=exact)
                    assert bf.stat("mfma") == 1 and int(ref[2].abs().sum().item()) == 0, tag
                    assert _same(got, ref), tag
    finally:
        ix.close()
        bf.close()


# ------------------------------------------------------------------------------------------------
# 3. off by default; the threshold; few queries, manhattan
# ------------------------------------------------------------------------------------------------
def test_off_by_default_and_the_threshold():
    import torch
    from hyperdb._native import METRIC_IDS
    Vb, Vw, Qall, _, _ = _case(384)
    mid, k = METRIC_IDS["cosine_similarity"], 50
    ix = _index(Vb, lds=None)
    try:
        assert ix.stat("f8_lds_min_q") == 0              # a fresh index: never
        ix.topk_device(Qall[:130], k, mid)
        assert ix.stat("f8_lds") == 0 and ix.stat("mfma") == 1
        ix.set_option("f8_lds_min_q", -1)                 # the measured rule: whatever it says, the stat reports it
        rule = ix.stat("f8_lds_min_q")
        assert rule == 0 or rule >= 5
        ix.set_option("f8_lds_min_q", 3)
        assert ix.stat("f8_lds_min_q") == 5               # never below the first batch size the matrix cores take
        ix.set_option("f8_lds_min_q", 33)
        assert ix.stat("f8_lds_min_q") == 33
        a32 = ix.topk_device(Qall[:32], k, mid)
        assert ix.stat("f8_lds") == 0 and ix.stat("mfma") == 1
        a33 = ix.topk_device(Qall[:33], k, mid)
        assert ix.stat("f8_lds") == 1 and ix.stat("mfma") == 1
        assert torch.equal(a32[0], a33[0][:32]) and torch.equal(a32[1].view(torch.int32), a33[1][:32].view(torch.int32))
        ix.set_option("f8_lds_min_q", 1)
        for nq in (1, 4):                                 # one VALU pass, whatever the option says
            ix.topk_device(Qall[:nq], k, mid)
            assert ix.stat("f8_lds") == 0 and ix.stat("mfma") == 0, nq
        ix.topk_device(Qall[:16], k, METRIC_IDS["manhattan_distance"])
        assert ix.stat("f8_lds") == 0 and ix.stat("mfma") == 0
    finally:
        ix.close()


def test_four_and_eight_waves_return_the_same_bits():
    """f8_lds_waves: 0 picks four waves for launches of up to 64 queries and eight beyond; 4 and 8 fix the count (d = 512 is built for
    four only).  The answer does not depend on it."""
    from hyperdb._native import METRIC_IDS
    mid, k = METRIC_IDS["cosine_similarity"], 50
    for d in (384, 512):
        Vb, _, Qall, _, _ = _case(d)
        ix = _index(Vb, 3)
        try:
            for nq in (17, 130):
                for exact in (False, True):
                    auto = _both(ix, Qall[:nq], k, mid, exact, (d, nq, exact))
                    for waves in (4, 8):
                        ix.set_option("f8_lds_waves", waves)
                        got = ix.topk_device(Qall[:nq], k, mid, exact=exact)
                        ix.set_option("f8_lds_waves", 0)
                        assert ix.stat("f8_lds") == 1 and _same(got, auto), (d, nq, exact, waves)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------
# 4. non-finite values are inputs, not faults
# ------------------------------------------------------------------------------------------------
def test_nan_code_keeps_the_matrix_off_the_matrix_cores():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    Vb, _, Qall, _, _ = _case(384)
    W = Vb.view(torch.uint8).clone()
    W[777, 300] = 0x7F
    ix = GpuIndex(W.view(torch.float8_e4m3fn))
    try:
        ix.set_option("max_blocks", 8)
        ix.set_option("f8_lds_min_q", 5)
        assert ix.has_nan
        i1, s1, st = ix.topk_device(Qall[:64], 20, METRIC_IDS["dot_product"])
        assert ix.stat("mfma") == 0 and ix.stat("f8_lds") == 0 and int(st.abs().sum().item()) == 0
        assert not bool((i1 == 777).any().item())         # NaN -> -inf: the row is never among the best
    finally:
        ix.close()


def test_infinite_query_elements_equal_the_register_flavour():
    import torch
    from hyperdb._native import METRIC_IDS
    Vb, _, Qall, _, _ = _case(384)
    Q = Qall[:64].copy()
    for j, qi in enumerate(range(0, 64, 8)):
        Q[qi, 11 + 45 * j] = np.inf if j % 2 == 0 else -np.inf
    mid, k = METRIC_IDS["dot_product"], 20
    ix = _index(Vb)
    try:
        # sampled: a list that overflowed (+inf on half of the rows) is answered by the exact re-run inside the call
        li, ls, lst = (x.copy() for x in ix.topk_views(Q, k, mid))
        ix.set_option("f8_lds_min_q", 0)
        ri, rs, rst = (x.copy() for x in ix.topk_views(Q, k, mid))
        ix.set_option("f8_lds_min_q", 5)
        assert np.array_equal(li, ri) and np.array_equal(ls.view(np.uint32), rs.view(np.uint32)) and np.array_equal(lst, rst)
        lds = ix.topk_device(Q, k, mid, exact=True)
        assert ix.stat("f8_lds") == 1 and ix.stat("mfma") == 1
        ix.set_option("f8_lds_min_q", 0)
        reg = ix.topk_device(Q, k, mid, exact=True)
        assert ix.stat("f8_lds") == 0 and _same(lds, reg)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# 5. lifecycle
# ------------------------------------------------------------------------------------------------
def test_append_and_compact_equal_a_fresh_index():
    import torch
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 256
    Vb, Vw, Qall, _, _ = _case(d)
    rng = np.random.default_rng(12)
    extra32 = rng.standard_normal((3_001, d)).astype(np.float32)
    extra_b, extra_w = _f8(extra32)
    Q = Qall[:65]
    n0 = 9_000
    ix = GpuIndex(Vb.view(torch.uint8)[:n0].clone().view(torch.float8_e4m3fn))
    try:
        ix.set_option("f8_lds_min_q", 5)
        ix.append(extra32[:1])
        ix.append(extra32[1:])
        assert ix.n == n0 + 3_001
        keep = np.flatnonzero(rng.random(ix.n) < 0.9)
        ix.compact(keep)
        assert ix.n == keep.size > 8192
        whole = torch.cat([Vb.view(torch.uint8)[:n0], extra_b.view(torch.uint8)])
        fresh = GpuIndex(whole[torch.from_numpy(keep).cuda()].contiguous().view(torch.float8_e4m3fn))
        try:
            fresh.set_option("f8_lds_min_q", 5)
            assert np.array_equal(ix.host_matrix(), fresh.host_matrix())
            a = ix.topk_device(Q, 30, METRIC_IDS["cosine_similarity"])
            m1 = ix.stat("f8_lds")
            b = fresh.topk_device(Q, 30, METRIC_IDS["cosine_similarity"])
            assert m1 == 1 and fresh.stat("f8_lds") == 1
            assert _same(a, b)
        finally:
            fresh.close()
    finally:
        ix.close()
