"""Batches of 5+ dot / cosine queries through the automatic int8 shadow (hdb_quant_mfma.hip, options quant_batch_min_n and
quant_batch_kernel).

The promise is the one of the 1-4-query flavour (tests/test_auto_quant.py): indices AND float32 score bits equal those of the same
index with use_quant = 0 and those of exact=True; a query whose floor check fails or whose list overflows says so in its status
word and the host entry re-runs it exactly.  quant_batch_kernel = 1 (int8 matrix cores) and 0 (the v_dot4 scan, four queries per
pass) are two independent filter kernels and must agree with the parent and with each other.
"""
import numpy as np
import pytest

from hyperdb import _native

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
# the measured default rule (quant_batch_rule, hdb_api.hip) at d = 384: 5 .. 16 queries from BATCH_MIN_ROWS rows on (17 .. 24 from
# 5M rows; no larger batch, no other width below 10M rows)
BATCH_MIN_ROWS = 3_000_000
BATCH_MIN_Q = 5
BATCH_MAX_Q = 16


def _torch():
    import torch
    return torch


def _matrix(n, d, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)


def _queries(nq, d, seed):
    return np.random.default_rng(seed).standard_normal((nq, d)).astype(np.float32)      # not fp16-representable


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _same(a_idx, a_sc, b_idx, b_sc):
    return np.array_equal(np.asarray(a_idx), np.asarray(b_idx)) and np.array_equal(_bits(a_sc), _bits(b_sc))


def _call(ix, Q, k, metric, exact=False):
    idx, sc, st = ix.topk_device(Q, k, M[metric], exact=exact)
    return idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()


def _stats(ix):
    return {s: ix.stat(s) for s in ("quant", "mfma", "path", "fused", "local")}


def _shadow_call(ix, Q, k, metric, kernel, what):
    ix.set_option("quant_batch_kernel", kernel)
    try:
        idx, sc, st = _call(ix, Q, k, metric)
        assert ix.stat("quant") == 1 and ix.stat("quant_auto") == 1, f"{what}: the call did not take the automatic shadow"
        assert ix.stat("mfma") == 1 and ix.stat("path") == 1 and ix.stat("fused") == 0, f"{what}: {_stats(ix)}"
        assert ix.stat("chunks") == (len(Q) + 255) // 256, f"{what}: {ix.stat('chunks')} chunks"
        assert (st == 0).all(), f"{what}: kernel {kernel}: status {st}"
        cands = ix.stat("quant_cands")
        assert k <= cands <= 8192, f"{what}: kernel {kernel}: {cands} candidates"
    finally:
        ix.set_option("quant_batch_kernel", 1)
    return idx, sc, cands


def _check_case(ix, Q, k, metric, what="", kernels=(1,)):
    got = {kernel: _shadow_call(ix, Q, k, metric, kernel, what) for kernel in kernels}
    idx, sc, cands = got[kernels[0]]
    for kernel in kernels[1:]:
        assert _same(idx, sc, got[kernel][0], got[kernel][1]), f"{what}: quant_batch_kernel {kernels[0]} and {kernel} differ"
    ix.set_option("use_quant", 0)
    try:
        pi, ps, pst = _call(ix, Q, k, metric)
        assert ix.stat("quant") == 0
    finally:
        ix.set_option("use_quant", 1)
    # (a default-path call whose own sampled threshold failed says so in its status word and its answer is the exact re-run's)
    assert not (pst == 0).all() or _same(idx, sc, pi, ps), f"{what}: differs from the default path (use_quant = 0)"
    ei, es, est = _call(ix, Q, k, metric, exact=True)
    assert ix.stat("quant") == 0
    assert (est == 0).all() and _same(idx, sc, ei, es), f"{what}: differs from exact=True"
    return cands


# ---------------------------------------------------------------------------------------------- 1. bit identity sweep
NQS = (5, 8, 16, 17, 33, 64, 128, 129, 256)
SHAPES = [(d, n) for d in (128, 256, 384, 512) for n in (20_000, 1_000_000)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", SHAPES, ids=[f"d{d}-n{n}" for d, n in SHAPES])
def test_bit_identity_with_the_default_path(d, n):
    torch = _torch()
    V = _matrix(n, d, seed=d + n)
    g = torch.Generator(device="cuda").manual_seed(7)
    bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
    mask = (torch.rand(n, generator=g, device="cuda") < 0.05).to(torch.uint8)
    ks = (1, 10, 100, 128)
    variants = ("plain", "bias", "mask", "both")
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("quant_batch_min_n", 0)
        assert ix.stat("quant_auto") == 0 and ix.stat("quant_bytes") == 0           # nothing until the first eligible call
        rot = (d // 128) + (n > 100_000)
        for case, nq in enumerate(NQS):
            metric = METRICS[(case + rot) % 2]
            variant = variants[(case // 2 + rot) % 4]
            k = ks[(case + case // 4 + rot) % 4]
            Q = _queries(nq, d, seed=case + d + 1000)
            b = bias if variant in ("bias", "both") else None
            m = mask if variant in ("mask", "both") else None
            if metric == "dot_product" and b is not None:
                b = b * 20.0
            ix.set_bias(b)
            ix.set_row_mask(m)
            cands = _check_case(ix, Q, k, metric, what=f"n={n} d={d} {metric} {variant} nq={nq} k={k}",
                                kernels=(1, 0) if nq in (8, 64, 256) else (1,))
            print(f"n={n} d={d} {metric} {variant} nq={nq} k={k}: largest list {cands}")
            ix.set_bias(None)
            ix.set_row_mask(None)
        assert ix.stat("quant_bytes") == n * (d + 12)
    finally:
        ix.close()
        del V
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 2. more than 256 queries
@pytest.mark.gpu
def test_more_than_256_queries_go_in_chunks():
    n, d = 100_000, 384
    V = _matrix(n, d, seed=41)
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("quant_batch_min_n", 0)
        Q = _queries(300, d, seed=42)
        for metric in METRICS:
            _check_case(ix, Q, 100, metric, what=f"300 queries {metric}", kernels=(1, 0))
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- 3. the default rule
@pytest.mark.gpu
def test_default_options_above_the_rule():
    torch = _torch()
    n, d = BATCH_MIN_ROWS + 100_000, 384
    V = _matrix(n, d, seed=5)
    ix = _native.GpuIndex(V)
    plain = _native.GpuIndex(V)
    try:
        plain.set_option("auto_quant", 0)
        for nq in (BATCH_MIN_Q, 8, BATCH_MAX_Q):
            for metric in METRICS:
                _check_case(ix, _queries(nq, d, seed=100 + nq), 100, metric, what=f"default options {metric} nq={nq}")
        # four queries: still the 1-4-query flavour (sample of 16)
        idx, sc, st = _call(ix, _queries(4, d, seed=104), 10, "cosine_similarity")
        assert ix.stat("quant") == 1 and ix.stat("mfma") == 1 and ix.stat("sample_m") == 16 and (st == 0).all()
        # query counts the rule excludes (measured slower than the fp16 single launch) keep the parent's path and statistics
        for nq in (BATCH_MAX_Q + 1, 64, 256):
            Q = _queries(nq, d, seed=105 + nq)
            idx, sc, st = _call(ix, Q, 10, "dot_product")
            got = _stats(ix)
            pi, ps, pst = _call(plain, Q, 10, "dot_product")
            assert got["quant"] == 0 and got == _stats(plain), (nq, got, _stats(plain))
            assert _same(idx, sc, pi, ps), nq
    finally:
        ix.close()
        plain.close()
        del V
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 4. adversarial data
def _host_index(Vh):
    ix = _native.GpuIndex(Vh)
    ix.set_option("quant_batch_min_n", 0)
    return ix


@pytest.mark.gpu
def test_duplicates_straddling_kth_of_three_queries():
    rng = np.random.default_rng(1)
    V = rng.standard_normal((50000, 384)).astype(np.float16)
    Q = rng.standard_normal((16, 384)).astype(np.float32)
    k = 100
    for j, qi in enumerate((2, 7, 13)):
        order = np.argsort(-(V.astype(np.float32) @ Q[qi]), kind="stable")
        V[order[k - 3:k + 3]] = V[order[k - 3]]              # six identical rows around the k-th place of this query ...
        V[[5 + j, 49990 - j]] = V[order[k - 3]]              # ... and two more far apart (tie order = row order)
    ix = _host_index(V)
    try:
        for metric in METRICS:
            _check_case(ix, Q, k, metric, what=f"duplicates {metric}", kernels=(1, 0))
    finally:
        ix.close()


@pytest.mark.gpu
def test_near_ties_below_int8_resolution():
    rng = np.random.default_rng(2)
    n, d = 40000, 384
    V = rng.standard_normal((n, d)).astype(np.float32)
    base = V[123].copy()
    s_r = np.abs(base).max() / 127.0
    rows = rng.choice(n, 300, replace=False)
    V[rows] = base + 1e-2 * s_r * rng.standard_normal((300, d)).astype(np.float32)       # (fp16 keeps differences of this size)
    V = V.astype(np.float16)
    Q = (base + 0.01 * rng.standard_normal((16, d))).astype(np.float32)
    ix = _host_index(V)
    plain = _native.GpuIndex(V)
    try:
        plain.set_option("auto_quant", 0)
        for metric in METRICS:
            idx, sc, st = _call(ix, Q, 100, metric)
            assert ix.stat("quant") == 1 and ix.stat("mfma") == 1 and ix.stat("fused") == 0
            ei, es, est = _call(ix, Q, 100, metric, exact=True)
            ok = st == 0
            assert _same(idx[ok], sc[ok], ei[ok], es[ok]), metric
            # through the host entry point too (its exact re-run covers a failed floor check)
            hi, hs = ix.topk(Q, 100, M[metric])
            pi, ps = plain.topk(Q, 100, M[metric])
            assert plain.stat("quant") == 0
            assert _same(hi, hs, ei, es) and _same(hi, hs, pi, ps), metric
    finally:
        ix.close()
        plain.close()


@pytest.mark.gpu
def test_one_huge_row_at_the_boundary():
    rng = np.random.default_rng(3)
    n, d, k = 30000, 384, 100
    V = rng.standard_normal((n, d)).astype(np.float16)
    Q = rng.standard_normal((16, d)).astype(np.float32)
    Q[:, 5] = 0.0
    order = np.argsort(-(V.astype(np.float32) @ Q[9]), kind="stable")
    j = 777
    V[j] = V[order[k - 1]]
    V[j, 5] = 400.0                                      # s_r is this one element: every other code rounds to ~0
    ix = _host_index(V)
    try:
        for metric in METRICS:
            _check_case(ix, Q, k, metric, what=f"huge row {metric}", kernels=(1, 0))
        idx, sc, st = _call(ix, Q, k, "dot_product")
        assert j in set(idx[9].tolist()) or order[k - 1] in set(idx[9].tolist())
    finally:
        ix.close()


@pytest.mark.gpu
def test_candidate_overflow_reruns_exactly():
    rng = np.random.default_rng(4)
    n, d = 20000, 384
    base = rng.standard_normal(d).astype(np.float32)
    V = (base + 1e-3 * rng.standard_normal((n, d))).astype(np.float16)      # near-identical rows: everything is a candidate
    Q = rng.standard_normal((16, d)).astype(np.float32)
    ix = _host_index(V)
    plain = _native.GpuIndex(V)
    try:
        plain.set_option("auto_quant", 0)
        for kernel in (1, 0):
            ix.set_option("quant_batch_kernel", kernel)
            idx, sc, st = _call(ix, Q, 100, "cosine_similarity")
            assert ix.stat("quant") == 1 and ix.stat("fused") == 0
            assert ((st & (_native.Q_OVERFLOW | _native.Q_UNDERFLOW)) != 0).all(), f"kernel {kernel}: every overflow must be reported: {st}"
            hi, hs = ix.topk(Q, 100, M["cosine_similarity"])
            assert ix.stat("quant") == 1                         # ("quant" reports the call's first attempt)
            pi, ps = plain.topk(Q, 100, M["cosine_similarity"])
            assert _same(hi, hs, pi, ps), kernel
    finally:
        ix.close()
        plain.close()


def _lattice(rng, rows, d, exps):
    """Integer codes in [-127, 127] with one +-127 per row, times a power of two per row: exact fp16 values that are exact
    multiples of their own scale max|x| / 127, so the quantization error of every row (and query) is zero."""
    C = rng.integers(-127, 128, size=(rows, d)).astype(np.float64)
    C[np.arange(rows), rng.integers(0, d, size=rows)] = 127.0 * rng.choice([-1.0, 1.0], size=rows)
    return C * np.exp2(rng.choice(exps, size=rows))[:, None]


@pytest.mark.gpu
@pytest.mark.parametrize("d,nq", [(384, 16), (128, 37), (512, 5)])
def test_lattice_data_leaves_no_room_for_a_wrong_operand_map(d, nq):
    rng = np.random.default_rng(50 + d)
    n = 40_000
    V = _lattice(rng, n, d, (-9.0, -8.0, -7.0, -6.0)).astype(np.float16)
    Q = _lattice(rng, nq, d, (-3.0, -2.0, 0.0, 1.0)).astype(np.float32)
    assert len({q.tobytes() for q in Q}) == nq and not (V[:-16] == V[16:]).all(axis=1).any()
    ix = _host_index(V)
    try:
        for metric in METRICS:
            for k in (10, 128):
                _check_case(ix, Q, k, metric, what=f"lattice d={d} {metric} k={k}", kernels=(1, 0))
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- 5. mixed batch
@pytest.mark.gpu
def test_batch_with_an_infinite_and_a_nan_query():
    n, d = 60_000, 384
    V = _matrix(n, d, seed=61)
    Q = _queries(16, d, seed=62)
    Q[3, 17] = np.inf
    Q[11, 200] = np.nan
    ix = _native.GpuIndex(V)
    plain = _native.GpuIndex(V)
    try:
        ix.set_option("quant_batch_min_n", 0)
        ix.set_option("quant_min_n", 0)
        plain.set_option("auto_quant", 0)
        good = np.array([q not in (3, 11) for q in range(16)])
        for metric in METRICS:
            one = {q: _call(ix, Q[q:q + 1], 10, metric)[2][0] for q in (3, 11)}      # what the 1-4-query flavour reports
            assert ix.stat("quant") == 1 and ix.stat("sample_m") == 16
            for kernel in (1, 0):
                ix.set_option("quant_batch_kernel", kernel)
                idx, sc, st = _call(ix, Q, 10, metric)
                assert ix.stat("quant") == 1 and ix.stat("fused") == 0 and ix.stat("sample_m") != 16
                assert st[3] == one[3] and (st[3] & _native.Q_UNDERFLOW), (metric, kernel, st)
                assert st[11] == one[11] and (st[11] & _native.Q_NAN), (metric, kernel, st)
                assert (st[good] == 0).all(), (metric, kernel, st)
                ei, es, est = _call(ix, Q[good], 10, metric, exact=True)
                assert _same(idx[good], sc[good], ei, es), (metric, kernel)
                # the host entry: a NaN query is an error on both indexes (the reference's message), the other fifteen -- the
                # infinite one re-run exactly -- equal a plain index
                for index in (ix, plain):
                    with pytest.raises(ValueError):
                        index.topk(Q, 10, M[metric])
                finite = np.arange(16) != 11
                hi, hs = ix.topk(Q[finite], 10, M[metric])
                assert ix.stat("quant") == 1
                pi, ps = plain.topk(Q[finite], 10, M[metric])
                assert plain.stat("quant") == 0 and _same(hi, hs, pi, ps), (metric, kernel)
            ix.set_option("quant_batch_kernel", 1)
    finally:
        ix.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- 6. not eligible
def _parent_stats(V, Q, k, metric, **options):
    """Answer and path statistics with the automatic shadow switched off: what the parent commit does."""
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("auto_quant", 0)
        for name, value in options.items():
            ix.set_option(name, value)
        idx, sc, st = _call(ix, Q, k, metric)
        return idx, sc, st, _stats(ix)
    finally:
        ix.close()


def _assert_parent_path(ix, V, Q, k, metric, what, **options):
    for name, value in options.items():
        ix.set_option(name, value)
    idx, sc, st = _call(ix, Q, k, metric)
    got = _stats(ix)
    pi, ps, pst, want = _parent_stats(V, Q, k, metric, **options)
    assert got["quant"] == 0 and got == want, (what, got, want)
    assert _same(idx, sc, pi, ps), what
    assert ix.stat("quant_auto") == 0 and ix.stat("quant_bytes") == 0, f"{what}: a call that is not eligible must not build the shadow"


@pytest.mark.gpu
def test_not_eligible_calls_keep_the_parent_path():
    torch = _torch()
    n, d = 60_000, 384
    V = _matrix(n, d, seed=21)
    Q = _queries(8, d, seed=22)
    ix = _native.GpuIndex(V)
    try:
        _assert_parent_path(ix, V, Q, 10, "cosine_similarity", "quant_batch_min_n unset on a small index")
        ix.set_option("quant_min_n", 0)
        _assert_parent_path(ix, V, Q, 10, "cosine_similarity", "quant_min_n does not govern batches")
        ix.set_option("quant_batch_min_n", 0)
        _assert_parent_path(ix, V, Q, 10, "euclidean_metric", "euclidean")
        _assert_parent_path(ix, V, Q, 200, "dot_product", "k = 200")
        _assert_parent_path(ix, V, Q, 10, "dot_product", "auto_quant = 0", auto_quant=0)
        ix.set_option("auto_quant", 1)
        _assert_parent_path(ix, V, Q, 10, "cosine_similarity", "use_mfma = 0", use_mfma=0)
        ix.set_option("use_mfma", 1)
        _check_case(ix, Q, 10, "cosine_similarity", what="eligible")          # ... and the same call is eligible otherwise
    finally:
        ix.close()
    # an explicit shadow keeps its own rule: batches stay on the parent's path
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("quant_batch_min_n", 0)
        ix.quantize("int8")
        idx, sc, st = _call(ix, Q, 10, "cosine_similarity")
        got = _stats(ix)
        pi, ps, pst, want = _parent_stats(V, Q, 10, "cosine_similarity")
        assert got["quant"] == 0 and got == want and ix.stat("quant_auto") == 0 and _same(idx, sc, pi, ps)
    finally:
        ix.close()
    # float32 matrix; a width the kernel does not take (d = 192: no whole geometry of the fp16 scan); d = 768 under the default rule
    for what, Vx, opts in (("float32", V.to(torch.float32), {"quant_batch_min_n": 0}),
                           ("d = 192", _matrix(n, 192, seed=23), {"quant_batch_min_n": 0}),
                           ("d = 768, default rule", _matrix(BATCH_MIN_ROWS + 1000, 768, seed=24), {}),
                           ("below the row rule", _matrix(BATCH_MIN_ROWS - 1000, 384, seed=26), {})):
        ix = _native.GpuIndex(Vx)
        try:
            for name, value in opts.items():
                ix.set_option(name, value)
            _assert_parent_path(ix, Vx, _queries(8, Vx.shape[1], seed=25), 10, "cosine_similarity", what)
        finally:
            ix.close()
            del Vx
            torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- 7. lifecycle
@pytest.mark.gpu
def test_append_update_compact_on_a_shadow_a_batch_built():
    rng = np.random.default_rng(6)
    n, d = 30000, 384
    V = rng.standard_normal((n, d)).astype(np.float16)
    Q = rng.standard_normal((8, d)).astype(np.float32)
    ix = _host_index(V)

    def fresh_equal(what, metric):
        idx, sc, st = _call(ix, Q, 100, metric)
        assert ix.stat("quant") == 1 and (st == 0).all(), what
        f = _native.GpuIndex(ix.V.clone())
        try:
            f.set_option("auto_quant", 0)
            fi, fs, fst = _call(f, Q, 100, metric)
            assert f.stat("quant") == 0 and _same(idx, sc, fi, fs), f"{what}: differs from a fresh index over the same rows"
        finally:
            f.close()

    try:
        _check_case(ix, Q, 100, "cosine_similarity", what="before append")
        assert ix.stat("quant_auto") == 1                    # built by the batch call
        new = (Q[0] + 0.05 * rng.standard_normal((40, d))).astype(np.float16)   # all belong in the top-k of query 0
        ix.append(new)
        idx, sc, st = _call(ix, Q, 100, "cosine_similarity")
        assert set(range(n, n + 40)) <= set(idx[0].tolist())
        _check_case(ix, Q, 100, "cosine_similarity", what="after append")
        fresh_equal("after append", "cosine_similarity")
        ix.append(rng.standard_normal((5000, d)).astype(np.float16))         # a second append (capacity growth)
        _check_case(ix, Q, 100, "dot_product", what="after second append")
        keep = np.sort(rng.choice(ix.n, 25000, replace=False))
        ix.compact(keep)
        _check_case(ix, Q, 100, "cosine_similarity", what="after compaction")
        fresh_equal("after compaction", "cosine_similarity")
        ix.update(-ix.V.clone())                             # a stale shadow would filter by the old rows
        _check_case(ix, Q, 100, "cosine_similarity", what="after update (negated)")
        _check_case(ix, Q, 100, "dot_product", what="after update (negated, dot)")
        fresh_equal("after update", "dot_product")
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- 8. the counter hand-out at d = 384
@pytest.mark.gpu
def test_batched_filter_pass_tiles_from_a_counter_without_the_shadow():
    """tests/test_gpu_parity.py::test_batched_filter_pass_tiles_from_a_counter[6000001-384-17-cosine_similarity] with use_quant = 0:
    a 17-query call on 6M x 384 rows rides the shadow by default, so the hand-out of the fp16 filter pass's tiles from a global
    counter is exercised at d = 384 here -- same candidates as the static split, so the same result bit for bit, with and without
    a bias, ragged last tile included; and both equal the on-device exact selection."""
    import bench
    torch = _torch()
    n, d, nq, metric = 6_000_001, 384, 17, "cosine_similarity"
    dev = torch.device("cuda", 0)
    V, _, _ = bench.make_shard(n, d, torch.float16, 0, 1, dev)
    V[n - 1] = V[5]                                         # the ragged last tile holds a row that ties with an early one
    Q = bench.make_queries(nq, d, torch.float16, dev).float()
    Q[1] = V[5].float()
    g = torch.Generator(device=dev).manual_seed(n)
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("use_quant", 0)
        mid = M[metric]
        for with_bias in (False, True):
            ix.set_bias((torch.rand(n, generator=g, device=dev) * 0.05).float() if with_bias else None)
            ix.set_option("dyn_tiles", 1)
            di, ds, dst = ix.topk_device(Q, 100, mid)
            assert ix.stat("quant") == 0 and ix.stat("mfma") == 1 and ix.stat("path") == 1 and ix.stat("fused") == 2
            assert int(dst.abs().sum().item()) == 0
            ix.set_option("dyn_tiles", 0)
            si, ss, sst = ix.topk_device(Q, 100, mid)
            ix.set_option("dyn_tiles", 1)
            assert int(sst.abs().sum().item()) == 0 and torch.equal(di, si) and torch.equal(ds, ss), with_bias
            ei, es, _ = ix.topk_device(Q[:6], 100, mid, exact=True)
            assert torch.equal(di[:6], ei) and torch.equal(ds[:6], es), with_bias
        assert ix.stat("quant_bytes") == 0
    finally:
        ix.close()
        del V
        torch.cuda.empty_cache()
