"""The automatic int8 shadow (option auto_quant, hdb_quant.hip "matrix-core flavour").

A default fp16 index answers 1-4 dot / cosine queries on the matrix cores.  From the automatic row threshold on (or with
quant_min_n set) such a call builds an int8 shadow on first use, filters on one byte per element and rescores the survivors with
the matrix-core MODE 0 launch.  The promise is bit identity with the default path: indices AND float32 score bits equal those of
the same index with use_quant = 0 and those of exact=True.  Calls that are not eligible keep the parent's path statistics.
"""
import numpy as np
import pytest

from hyperdb import _native

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
AUTO_MIN_ROWS = 2_000_000          # HDB_QUANT_AUTO_MIN_ROWS (hdb_api.hip)


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


def _check_case(ix, Q, k, metric, what=""):
    idx, sc, st = _call(ix, Q, k, metric)
    assert ix.stat("quant") == 1 and ix.stat("quant_auto") == 1, f"{what}: the call did not take the automatic shadow"
    assert ix.stat("mfma") == 1 and ix.stat("path") == 1 and ix.stat("fused") == 0, f"{what}: {_stats(ix)}"
    assert (st == 0).all(), f"{what}: status {st}"
    cands = ix.stat("quant_cands")
    assert k <= cands <= 8192, f"{what}: {cands} candidates"
    ix.set_option("use_quant", 0)
    try:
        pi, ps, pst = _call(ix, Q, k, metric)
        assert ix.stat("quant") == 0
    finally:
        ix.set_option("use_quant", 1)
    # (a default-path call whose own sampled threshold failed says so in its status word and its answer is the exact re-run's: (b))
    assert not (pst == 0).all() or _same(idx, sc, pi, ps), f"{what}: differs from the default path (use_quant = 0)"
    ei, es, est = _call(ix, Q, k, metric, exact=True)
    assert ix.stat("quant") == 0
    assert (est == 0).all() and _same(idx, sc, ei, es), f"{what}: differs from exact=True"
    return cands


def _sweep(ix, n, d):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(7)
    bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
    mask = (torch.rand(n, generator=g, device="cuda") < 0.05).to(torch.uint8)
    ks = (1, 10, 100, 128)
    case = 0
    for metric in METRICS:
        for variant in ("plain", "bias", "mask", "both"):
            nq = 1 + case % 4
            k = ks[(case // 4 + case) % 4]
            case += 1
            Q = _queries(nq, d, seed=case + d)
            b = bias if variant in ("bias", "both") else None
            m = mask if variant in ("mask", "both") else None
            if metric == "dot_product" and b is not None:
                b = b * 20.0
            ix.set_bias(b)
            ix.set_row_mask(m)
            _check_case(ix, Q, k, metric, what=f"n={n} d={d} {metric} {variant} nq={nq} k={k}")
            ix.set_bias(None)
            ix.set_row_mask(None)


SHAPES = [(d, n) for d in (128, 384, 768) for n in (20_000, 1_000_000)]


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", SHAPES, ids=[f"d{d}-n{n}" for d, n in SHAPES])
def test_bit_identity_with_the_default_path(d, n):
    V = _matrix(n, d, seed=d + n)
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("quant_min_n", 0)
        assert ix.stat("quant_auto") == 0 and ix.stat("quant_bytes") == 0           # nothing until the first eligible call
        _sweep(ix, n, d)
        assert ix.stat("quant_bytes") == n * (((d + 15) // 16) * 16 + 12)
    finally:
        ix.close()


@pytest.mark.gpu
def test_above_the_automatic_rule_with_default_options():
    torch = _torch()
    n, d = AUTO_MIN_ROWS + 100_000, 384
    V = _matrix(n, d, seed=5)
    ix = _native.GpuIndex(V)
    try:
        _sweep(ix, n, d)
        # every query count and every k once more on the plain index
        for nq in (1, 2, 3, 4):
            for k in (1, 10, 100, 128):
                for metric in METRICS:
                    _check_case(ix, _queries(nq, d, seed=100 + nq + k), k, metric, what=f"default options {metric} nq={nq} k={k}")
    finally:
        ix.close()
        del V
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------- adversarial data
def _host_index(Vh):
    ix = _native.GpuIndex(Vh)
    ix.set_option("quant_min_n", 0)
    return ix


@pytest.mark.gpu
def test_duplicates_straddling_kth():
    rng = np.random.default_rng(1)
    V = rng.standard_normal((50000, 384)).astype(np.float16)
    q = rng.standard_normal((1, 384)).astype(np.float32)
    k = 100
    order = np.argsort(-(V.astype(np.float32) @ q[0]), kind="stable")
    V[order[k - 3:k + 3]] = V[order[k - 3]]              # six identical rows around the k-th place ...
    V[[5, 49990]] = V[order[k - 3]]                      # ... and two more far apart (tie order = row order)
    ix = _host_index(V)
    try:
        for metric in METRICS:
            _check_case(ix, q, k, metric, what=f"duplicates {metric}")
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
    q = (base + 0.01 * rng.standard_normal(d)).astype(np.float32).reshape(1, d)
    ix = _host_index(V)
    plain = _native.GpuIndex(V)
    try:
        for metric in METRICS:
            idx, sc, st = _call(ix, q, 100, metric)
            assert ix.stat("quant") == 1 and ix.stat("mfma") == 1
            ei, es, est = _call(ix, q, 100, metric, exact=True)
            if (st == 0).all():
                assert _same(idx, sc, ei, es), metric
            # through the host entry point too (its exact re-run covers a failed floor check)
            hi, hs = ix.topk(q, 100, M[metric])
            pi, ps = plain.topk(q, 100, M[metric])
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
    q = rng.standard_normal(d).astype(np.float32)
    q[5] = 0.0
    order = np.argsort(-(V.astype(np.float32) @ q), kind="stable")
    j = 777
    V[j] = V[order[k - 1]]
    V[j, 5] = 400.0                                      # s_r is this one element: every other code rounds to ~0
    ix = _host_index(V)
    try:
        for metric in METRICS:
            _check_case(ix, q.reshape(1, d), k, metric, what=f"huge row {metric}")
        idx, sc, st = _call(ix, q.reshape(1, d), k, "dot_product")
        assert j in set(idx[0].tolist()) or order[k - 1] in set(idx[0].tolist())
    finally:
        ix.close()


@pytest.mark.gpu
def test_candidate_overflow_reruns_exactly():
    rng = np.random.default_rng(4)
    n, d = 20000, 384
    base = rng.standard_normal(d).astype(np.float32)
    V = (base + 1e-3 * rng.standard_normal((n, d))).astype(np.float16)      # near-identical rows: everything is a candidate
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _host_index(V)
    plain = _native.GpuIndex(V)
    try:
        idx, sc, st = _call(ix, q, 100, "cosine_similarity")
        assert ix.stat("quant") == 1
        assert st[0] & (_native.Q_OVERFLOW | _native.Q_UNDERFLOW), "the overflow must be reported on the device API"
        hi, hs = ix.topk(q, 100, M["cosine_similarity"])
        assert ix.stat("quant") == 1                         # ("quant" reports the call's first attempt)
        pi, ps = plain.topk(q, 100, M["cosine_similarity"])
        assert _same(hi, hs, pi, ps)
    finally:
        ix.close()
        plain.close()


# ---------------------------------------------------------------------------------------------- not eligible
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


@pytest.mark.gpu
def test_not_eligible_calls_keep_the_parent_path():
    torch = _torch()
    n, d = 60000, 384
    V = _matrix(n, d, seed=21)
    Q5 = _queries(5, d, seed=22)
    ix = _native.GpuIndex(V)
    try:
        # below the automatic rule, default options
        idx, sc, st = _call(ix, Q5[:1], 10, "cosine_similarity")
        want = _parent_stats(V, Q5[:1], 10, "cosine_similarity")
        assert ix.stat("quant") == 0 and _stats(ix) == want[3] and _same(idx, sc, want[0], want[1])
        ix.set_option("quant_min_n", 0)
        for what, Q, k, metric, opts in (
                ("euclidean", Q5[:2], 10, "euclidean_metric", {}),
                ("five queries", Q5, 10, "cosine_similarity", {}),
                ("k = 200", Q5[:1], 200, "dot_product", {}),
                ("auto_quant = 0", Q5[:3], 10, "dot_product", {"auto_quant": 0}),
                ("use_mfma = 0", Q5[:1], 10, "cosine_similarity", {"use_mfma": 0})):
            for name, value in opts.items():
                ix.set_option(name, value)
            idx, sc, st = _call(ix, Q, k, metric)
            got = _stats(ix)
            for name in opts:
                ix.set_option(name, 1)
            pi, ps, pst, want = _parent_stats(V, Q, k, metric, **opts)
            assert got["quant"] == 0 and got == want, (what, got, want)
            assert _same(idx, sc, pi, ps), what
        assert ix.stat("quant_auto") == 0 and ix.stat("quant_bytes") == 0, "a call that is not eligible must not build the shadow"
        # eligible now: builds it; quantize(None) drops it and switches the automatic build off for the handle
        _check_case(ix, Q5[:2], 10, "cosine_similarity", what="eligible")
        ix.quantize(None)
        idx, sc, st = _call(ix, Q5[:2], 10, "cosine_similarity")
        want = _parent_stats(V, Q5[:2], 10, "cosine_similarity")
        assert ix.stat("quant") == 0 and ix.stat("quant_bytes") == 0 and _stats(ix) == want[3] and _same(idx, sc, want[0], want[1])
    finally:
        ix.close()
    # float32 matrix
    Vf = V.to(torch.float32)
    ix = _native.GpuIndex(Vf)
    try:
        ix.set_option("quant_min_n", 0)
        idx, sc, st = _call(ix, Q5[:1], 10, "cosine_similarity")
        want = _parent_stats(Vf, Q5[:1], 10, "cosine_similarity")
        assert ix.stat("quant") == 0 and ix.stat("quant_bytes") == 0 and _stats(ix) == want[3] and _same(idx, sc, want[0], want[1])
    finally:
        ix.close()


@pytest.mark.gpu
def test_infinite_element_declines_and_leaves_no_shadow():
    rng = np.random.default_rng(9)
    V = rng.standard_normal((20000, 384)).astype(np.float16)
    V[77, 3] = np.inf
    q = rng.standard_normal((1, 384)).astype(np.float32)
    ix = _host_index(V)
    try:
        idx, sc, st = _call(ix, q, 50, "dot_product")
        got = _stats(ix)
        pi, ps, pst, want = _parent_stats(V, q, 50, "dot_product")
        assert got["quant"] == 0 and got == want and ix.stat("quant_bytes") == 0 and ix.stat("quant_auto") == 0
        assert _same(idx, sc, pi, ps)
    finally:
        ix.close()


@pytest.mark.gpu
def test_explicit_shadow_keeps_the_valu_bits():
    V = _matrix(30000, 384, seed=31)
    q = _queries(2, 384, seed=32)
    ix = _native.GpuIndex(V)
    try:
        ix.set_option("quant_min_n", 0)
        _check_case(ix, q, 10, "cosine_similarity", what="automatic first")
        ix.quantize("int8")                                  # explicit from here on
        idx, sc, st = _call(ix, q, 10, "cosine_similarity")
        assert ix.stat("quant") == 1 and ix.stat("mfma") == 0 and ix.stat("quant_auto") == 0
        ix.set_option("use_quant", 0); ix.set_option("use_mfma", 0); ix.set_option("use_fused", 0)
        pi, ps, pst = _call(ix, q, 10, "cosine_similarity")
        assert _same(idx, sc, pi, ps)
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- lifecycle
@pytest.mark.gpu
def test_append_update_compact_on_an_automatic_shadow():
    rng = np.random.default_rng(6)
    n, d = 30000, 384
    V = rng.standard_normal((n, d)).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _host_index(V)
    try:
        _check_case(ix, q, 100, "cosine_similarity", what="before append")
        new = (q[0] + 0.05 * rng.standard_normal((40, d))).astype(np.float16)   # all belong in the top-k
        ix.append(new)
        idx, sc, st = _call(ix, q, 100, "cosine_similarity")
        assert set(range(n, n + 40)) <= set(idx[0].tolist())
        _check_case(ix, q, 100, "cosine_similarity", what="after append")
        ix.append(rng.standard_normal((5000, d)).astype(np.float16))         # a second append (capacity growth)
        _check_case(ix, q, 100, "dot_product", what="after second append")
        keep = np.sort(rng.choice(ix.n, 25000, replace=False))
        ix.compact(keep)
        _check_case(ix, q, 100, "cosine_similarity", what="after compaction")
        ix.update(-ix.V.clone())                             # a stale shadow would filter by the old rows
        _check_case(ix, q, 100, "cosine_similarity", what="after update (negated)")
        _check_case(ix, q, 100, "dot_product", what="after update (negated, dot)")
    finally:
        ix.close()


# ---------------------------------------------------------------------------------------------- gamma_m, measured
def _rounded_query(q):
    """q' = fp16(q * scale) / scale with the library's power-of-two scale (hdb_q16_scale), in float64."""
    amax = float(np.abs(q).max())
    _, ex = np.frexp(np.float32(amax))
    scale = np.float32(2.0) ** int(15 - ex)
    q16 = (q.astype(np.float32) * scale).astype(np.float16)
    return q16.astype(np.float64) / float(scale)


@pytest.mark.gpu
@pytest.mark.parametrize("d", (128, 384, 768))
def test_gamma_m_measured(d):
    """|S_m - q'.v| / (||q'|| ||v||) of the matrix-core dot products against float64 dot products of the same fp16 values, random
    and adversarial rows; the bound (2m) of hdb_quant.hip assumes gamma_m = (d + 8) 2^-22 and this asserts a quarter of it.
    Observed maxima on MI355X: 2.7e-7 (d = 128), 4.3e-7 (d = 384), 8.2e-7 (d = 768) -- 0.8 %, 0.5 %, 0.4 % of gamma_m."""
    rng = np.random.default_rng(40 + d)
    blk, nblk = 2048, 10
    n = blk * nblk
    V = rng.standard_normal((n, d)).astype(np.float32)
    V[1 * blk:2 * blk] = np.abs(V[1 * blk:2 * blk])                                   # all the same sign
    V[2 * blk:3 * blk] = 65504.0 * np.sign(V[2 * blk:3 * blk])                        # every element at the fp16 maximum, random signs
    V[3 * blk:4 * blk] = 65504.0                                                      # ... all positive (one element per row differs:
    V[np.arange(3 * blk, 4 * blk), np.arange(blk) % d] = np.abs(rng.standard_normal(blk)).astype(np.float32) * 1000.0   # no 2048-way tie)
    alt = np.where(np.arange(d) % 2 == 0, 1000.0, 1e-3).astype(np.float32)
    V[4 * blk:5 * blk] = V[4 * blk:5 * blk] * alt                                     # alternating large / small
    V[5 * blk:6 * blk] = np.abs(V[5 * blk:6 * blk]) * alt
    V[6 * blk:7 * blk] = V[6 * blk:7 * blk] * np.float32(1e-4)                        # small magnitudes (fp16 subnormals among them)
    V = V.astype(np.float16)
    queries = [rng.standard_normal(d), np.abs(rng.standard_normal(d)), rng.standard_normal(d) * alt[::-1],
               np.abs(rng.standard_normal(d)) * alt, np.full(d, 0.3)]
    gamma_m = (d + 8) * 2.0 ** -22
    worst = 0.0
    ix = _native.GpuIndex(V)
    try:
        V64 = V.astype(np.float64)
        vnorm = np.linalg.norm(V64, axis=1)
        for q in queries:
            q = q.astype(np.float32).reshape(1, d)
            qr = _rounded_query(q[0])
            ref = V64 @ qr
            for b in range(nblk):
                mask = np.zeros(n, np.uint8)
                mask[b * blk:(b + 1) * blk] = 1
                ix.set_row_mask(mask)
                idx, sc, st = _call(ix, q, blk, "dot_product", exact=True)
                assert ix.stat("mfma") == 1 and (st == 0).all()
                rows = idx[0]
                assert rows.min() >= b * blk and rows.max() < (b + 1) * blk
                err = np.abs(sc[0].astype(np.float64) - ref[rows]) / (np.linalg.norm(qr) * vnorm[rows])
                worst = max(worst, float(err.max()))
        print(f"gamma_m measurement d={d}: observed max {worst:.3e}, assumed gamma_m {gamma_m:.3e} (ratio {worst / gamma_m:.4f})")
        assert worst <= gamma_m / 4
    finally:
        ix.close()
