"""The 5-bit plane of the int8 shadow on the GPU (hdb_quant.hip, "The 5-bit plane"; options use_plane, plane_min_n, plane_cap_rows).

A one-query dot / cosine call through the shadow first streams the high five bits of the codes and runs the int8 pass over the
surviving rows only.  The promise is identity: the candidate list, and therefore indices, score bits and status, are those of the
same call with use_plane = 0, which in turn are those of the call without the shadow.
"""
import numpy as np
import pytest

from hyperdb import _native

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
DIMS = (16, 40, 384, 512)
ROWS = (8209, 70001)                    # just above HDB_CAND_CAP; a ragged last tile both times
# The automatic shadow exists where a one-query fp16 call runs on the matrix cores: widths with a geometry of their own.  The other
# widths answer one query on the VALU scan and never build one (hdb_api.hip, min_q), so only the explicit shadow applies to them.
AUTO_DIMS = (384, 512)


def _torch():
    import torch
    return torch


def _matrix(n, d, dtype, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(dtype)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _raw(ix, Q, k, metric):
    idx, sc, st = ix.topk_device(Q, k, M[metric])
    return idx.cpu().numpy(), _bits(sc.cpu().numpy()), st.cpu().numpy()


def _host(ix, Q, k, metric):
    idx, sc = ix.topk(Q, k, M[metric])
    return np.asarray(idx), _bits(sc)


def _index(V, flavour):
    """flavour 'auto': the shadow the fp16 index builds itself (matrix-core bits); 'explicit': hdb_index_quantize (VALU bits: the
    index keeps to the VALU scan for everything else too, the exact re-run of a failed status included)."""
    ix = _native.GpuIndex(V)
    if flavour == "explicit":
        ix.quantize("int8")
        ix.set_option("use_mfma", 0)
        ix.set_option("use_fused", 0)
    ix.set_option("quant_min_n", 0)
    ix.set_option("plane_min_n", 0)
    return ix


class _Options:
    def __init__(self, ix, **opts):
        self.ix, self.opts = ix, opts

    def __enter__(self):
        for name, v in self.opts.items():
            self.ix.set_option(name, v)

    def __exit__(self, *exc):
        for name in self.opts:
            self.ix.set_option(name, 1)


def _no_shadow(ix):
    """The call without the shadow whose bits the index reproduces: the default path (auto) or the VALU scan (explicit, _index)."""
    return _Options(ix, use_quant=0)


def _identity(ix, flavour, Q, k, metric, what):
    on = _raw(ix, Q, k, metric)
    assert ix.stat("quant") == 1 and ix.stat("plane") == 1, f"{what}: the call did not take the plane"
    cands_on, surv = ix.stat("quant_cands"), ix.stat("plane_survivors")
    on_h = _host(ix, Q, k, metric)
    with _Options(ix, use_plane=0):
        off = _raw(ix, Q, k, metric)
        assert ix.stat("quant") == 1 and ix.stat("plane") == 0 and ix.stat("plane_survivors") == 0
        cands_off = ix.stat("quant_cands")
        off_h = _host(ix, Q, k, metric)
    assert cands_on == cands_off, f"{what}: {cands_on} candidates behind the plane, {cands_off} without it"
    assert surv >= cands_on, f"{what}: {surv} survivors, {cands_on} candidates"
    for a, b in zip(on, off):
        assert np.array_equal(a, b), f"{what}: plane on and off differ"
    with _no_shadow(ix):
        ref = _raw(ix, Q, k, metric)
        assert ix.stat("quant") == 0 and ix.stat("plane") == 0
        ref_h = _host(ix, Q, k, metric)
    assert np.array_equal(on[2], ref[2]), f"{what}: status {on[2]} with the shadow, {ref[2]} without"
    # A non-zero status (the mask that keeps fewer than k rows: no k-th candidate above the threshold) says that the device buffers
    # hold the failed attempt's partial list, which is each path's own and which hdb_topk_host discards for the exact re-run.  The
    # buffers are compared where the status is zero, the answers of the host entry -- what a caller gets -- always.
    if (ref[2] == 0).all():
        assert np.array_equal(on[0], ref[0]) and np.array_equal(on[1], ref[1]), f"{what}: differs from the call without the shadow"
    for a, b, c in zip(on_h, off_h, ref_h):
        assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: host answers differ"
    return surv


CASES = [(d, n, fl, dt) for d in DIMS for n in ROWS for fl, dt in (("auto", "f16"), ("explicit", "f16"), ("explicit", "f32"))
         if fl == "explicit" or d in AUTO_DIMS]


@pytest.mark.gpu
@pytest.mark.parametrize("d,n,flavour,dt", CASES, ids=[f"d{d}-n{n}-{fl}-{dt}" for d, n, fl, dt in CASES])
def test_identity(d, n, flavour, dt):
    torch = _torch()
    V = _matrix(n, d, torch.float16 if dt == "f16" else torch.float32, seed=d + n)
    ix = _index(V, flavour)
    try:
        g = torch.Generator(device="cuda").manual_seed(3)
        bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
        few = torch.zeros(n, dtype=torch.uint8, device="cuda")
        few[torch.randperm(n, generator=g, device="cuda")[:37]] = 1                  # fewer than k rows stay
        U = (((d + 15) // 16) * 16 + 31) // 32
        for mi, metric in enumerate(METRICS):
            for variant in ("plain", "bias", "mask"):
                Q = np.random.default_rng(d + mi).standard_normal((1, d)).astype(np.float32)
                ix.set_bias((bias * 20.0 if metric == "dot_product" else bias) if variant == "bias" else None)
                ix.set_row_mask(few if variant == "mask" else None)
                _identity(ix, flavour, Q, 100, metric, f"d={d} n={n} {flavour} {dt} {metric} {variant}")
                ix.set_bias(None)
                ix.set_row_mask(None)
        assert ix.stat("plane_bytes") == n * (20 * U + 16)
        assert ix.stat("quant_bytes") == n * (((d + 15) // 16) * 16 + 12)
    finally:
        ix.close()


@pytest.mark.gpu
def test_both_list_regimes():
    torch = _torch()
    n, d = 70001, 384
    V = _matrix(n, d, torch.float16, seed=17)
    Q = np.random.default_rng(17).standard_normal((1, d)).astype(np.float32)
    ix = _index(V, "auto")
    try:
        ix.set_option("plane_cap_rows", n)
        big = _raw(ix, Q, 100, "cosine_similarity")
        assert ix.stat("plane") == 1 and ix.stat("plane_overflows") == 0
        surv, cands = ix.stat("plane_survivors"), ix.stat("quant_cands")
        assert 16 < surv <= n
        ix.set_option("plane_cap_rows", 16)
        small = _raw(ix, Q, 100, "cosine_similarity")
        assert ix.stat("plane") == 1 and ix.stat("plane_overflows") == 1            # pass 2 scanned all rows
        assert ix.stat("plane_survivors") == surv and ix.stat("quant_cands") == cands
        small2 = _raw(ix, Q, 100, "cosine_similarity")
        assert ix.stat("plane_overflows") == 2
        for a, b, c in zip(big, small, small2):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert (big[2] == 0).all()
    finally:
        ix.close()


def _adversarial_rows(rng, d):
    """fp16 rows whose codes have every residual -4 (multiples of 8), every residual +3, all +-127, and a zero row: the largest
    element is 127 * 2^-5, so an element c * 2^-5 quantizes to the code c exactly."""
    h = rng.integers(-15, 15, size=(3, d))
    rows = [8 * h[0], 8 * h[1] + 7, 8 * h[2] + 7 * rng.integers(0, 2, size=d)]
    for r in rows:
        r[0] = 127
    rows += [np.full(d, 127), np.full(d, -127), np.where(rng.integers(0, 2, size=d) == 1, 127, -127), np.zeros(d, np.int64)]
    return (np.stack(rows).astype(np.float64) / 32.0).astype(np.float16)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_bound_on_the_device(d):
    rng = np.random.default_rng(d)
    n = 70001 if d == 384 else 8209
    Vh = rng.standard_normal((n, d)).astype(np.float16)
    adv = _adversarial_rows(rng, d)
    Vh[100:100 + adv.shape[0]] = adv
    queries = [rng.standard_normal(d).astype(np.float32)]
    codes = np.rint(adv[:3].astype(np.float64) * 32.0)
    rho = codes - (8 * np.floor(codes / 8) + 4)
    for r in range(3):
        queries.append((np.sign(rho[r]) * 1.0).astype(np.float32))                  # signs aligned with the residuals
        queries.append((-np.sign(rho[r]) * 1.0).astype(np.float32))
    one = np.zeros(d, np.float32); one[d // 3] = -2.5
    queries.append(one)
    bias = (rng.random(n) * 0.05).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    for flavour in (("auto", "explicit") if d in AUTO_DIMS else ("explicit",)):
        ix = _index(Vh, flavour)
        try:
            ix.topk_device(queries[0][None, :], 10, M["cosine_similarity"])         # (the automatic flavour builds its shadow here)
            assert ix.stat("plane") == 1
            for metric in METRICS:
                for variant in ("plain", "bias", "mask"):
                    ix.set_bias(bias if variant == "bias" else None)
                    ix.set_row_mask(mask if variant == "mask" else None)
                    for qi, q in enumerate(queries):
                        hi, hi5 = ix.quant_bounds(q, M[metric])
                        assert not np.isnan(hi5).any()
                        assert (hi5 >= hi).all(), f"d={d} {flavour} {metric} {variant} query {qi}: hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
                        if variant == "mask":
                            assert np.isneginf(hi5[mask == 0]).all() and np.isfinite(hi5[mask != 0]).all()
                    ix.set_bias(None)
                    ix.set_row_mask(None)
        finally:
            ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ("auto", "explicit"))
def test_maintenance(flavour):
    rng = np.random.default_rng(9)
    n, d = 30000, 384
    rowb = 20 * 12 + 16
    V = rng.standard_normal((n + 5040, d)).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)

    def check(ix, rows, what):
        got = _raw(ix, q, 100, "cosine_similarity")                              # (the automatic flavour builds its shadow on the first call)
        assert ix.stat("plane") == 1, what
        assert ix.stat("plane_bytes") == rows.shape[0] * rowb, what
        fresh = _index(rows, flavour)
        try:
            want = _raw(fresh, q, 100, "cosine_similarity")
            assert fresh.stat("plane") == 1
            assert ix.stat("plane_survivors") == fresh.stat("plane_survivors"), what
            assert ix.stat("quant_cands") == fresh.stat("quant_cands"), what
        finally:
            fresh.close()
        for a, b in zip(got, want):
            assert np.array_equal(a, b), what
        assert (got[2] == 0).all(), what

    ix = _index(V[:n].copy(), flavour)
    try:
        check(ix, V[:n], "fresh")
        near = (q[0] + 0.05 * rng.standard_normal((40, d))).astype(np.float16)       # all belong in the top-k
        V[n:n + 40] = near
        ix.append(V[n:n + 40])
        check(ix, V[:n + 40], "after extend")
        ix.append(V[n + 40:])                                                        # a second append (capacity growth)
        check(ix, V, "after the second extend")
        keep = np.sort(rng.choice(V.shape[0], 25000, replace=False))                 # remove + compaction
        ix.compact(keep)
        check(ix, V[keep], "after compaction")
        W = -V[keep][::-1].copy()
        ix.update(W)
        check(ix, W, "after update")
    finally:
        ix.close()


@pytest.mark.gpu
def test_extend_to_the_last_row_of_the_capacity():
    """An explicit shadow of n0 rows has room for n0 + n0 / 2 + 64; an extend to exactly that many (not a multiple of 16) leaves no
    spare row behind the ragged last tile of pass 1."""
    rng = np.random.default_rng(12)
    n0, d = 9000, 384
    cap = n0 + n0 // 2 + 64
    assert cap % 16 != 0
    V = rng.standard_normal((cap, d)).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)
    V[cap - 3:] = (q[0] + 0.05 * rng.standard_normal((3, d))).astype(np.float16)     # the last rows belong in the top-k
    ix = _index(V[:n0].copy(), "explicit")
    fresh = _index(V, "explicit")
    try:
        ix.append(V[n0:])
        assert ix.stat("plane_bytes") == cap * (20 * 12 + 16)
        got = _raw(ix, q, 100, "cosine_similarity")
        assert ix.stat("plane") == 1
        want = _raw(fresh, q, 100, "cosine_similarity")
        assert ix.stat("plane_survivors") == fresh.stat("plane_survivors") and ix.stat("quant_cands") == fresh.stat("quant_cands")
        for a, b in zip(got, want):
            assert np.array_equal(a, b)
        assert (got[2] == 0).all() and {cap - 3, cap - 2, cap - 1} <= set(got[0][0].tolist())
    finally:
        ix.close()
        fresh.close()


@pytest.mark.gpu
def test_ineligible_calls_keep_their_path():
    torch = _torch()
    n, d = 70001, 384
    V = _matrix(n, d, torch.float16, seed=23)
    rng = np.random.default_rng(23)
    ix = _index(V, "auto")
    ex = _index(V, "explicit")
    try:
        Q2 = rng.standard_normal((2, d)).astype(np.float32)
        for name, h in (("auto", ix), ("explicit", ex)):
            one = _raw(h, Q2[:1], 100, "cosine_similarity")
            assert h.stat("plane") == 1
            two = _raw(h, Q2, 100, "cosine_similarity")
            assert h.stat("quant") == 1 and h.stat("plane") == 0 and h.stat("plane_survivors") == 0, name
            assert h.stat("path") == 1 and h.stat("fused") == 0 and h.stat("mfma") == (1 if name == "auto" else 0)
            assert np.array_equal(two[0][0], one[0][0]) and np.array_equal(two[1][0], one[1][0])
        euc = _raw(ex, Q2[:1], 100, "euclidean_metric")
        assert ex.stat("quant") == 1 and ex.stat("plane") == 0 and ex.stat("mfma") == 0 and ex.stat("path") == 1
        with _Options(ex, use_quant=0):
            ref = _raw(ex, Q2[:1], 100, "euclidean_metric")
        for a, b in zip(euc, ref):
            assert np.array_equal(a, b)
        _raw(ix, Q2[:1], 100, "euclidean_metric")                                   # the automatic shadow never takes euclidean calls
        assert ix.stat("quant") == 0 and ix.stat("plane") == 0
    finally:
        ix.close()
        ex.close()
