"""The one-query shadow call whose plane pass does not stream the sampled tiles (hdb_quant.hip): the sample pass leaves MODE 1's upper
bound of every sampled row in a list, pass 1 walks the other tiles (hdb_plane_skip_*, hdb_caps.h) and queues the sampled rows with
!(hi < T_s) from the list.  The promise is unchanged: indices, score bits, status and the candidate count of a call behind the plane
are those of the call with use_plane = 0, and the answers those of the call without the shadow.

What can go wrong only here: a sampled row that is a winner reaches the answer through the list alone (winners planted only inside
sampled tiles -- the tile numbers from tile_index, the restatement of hdb_tile_index that tests/test_plane_skip_plan.py pins against
the library); the ragged last tile is never sampled and must still be walked (winners planted only there); a mask may remove every
sampled row (T_s = -inf: every live row is a candidate and no masked row may enter a queue); list chunks must refill queues that the
stream left nearly full (the near-copies matrix of tests/test_quant_inpass.py); and the folded threshold (hq_fold_thr, now DPP
reductions) must give the value it gave.  Shapes: the smallest the path takes (test_quant_inpass.py, "Shapes"), d = 200 for an odd
unit count, and the smallest n at which the threshold is folded into the passes, computed from the plan.
"""
import numpy as np
import pytest

from hyperdb import _native
from test_plane_skip_plan import tile_index

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")


def _torch():
    import torch
    return torch


def _matrix(n, d, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _raw(ix, Q, k, metric):
    idx, sc, st = ix.topk_device(Q, k, M[metric])
    return idx.cpu().numpy(), _bits(sc.cpu().numpy()), st.cpu().numpy()


def _host(ix, Q, k, metric):
    idx, sc = ix.topk(Q, k, M[metric])
    return np.asarray(idx), _bits(sc)


def _index(V, flavour="auto"):
    ix = _native.GpuIndex(V)
    if flavour == "explicit":
        ix.quantize("int8")
        ix.set_option("use_mfma", 0)
        ix.set_option("use_fused", 0)
    ix.set_option("quant_min_n", 0)
    ix.set_option("plane_min_n", 0)
    return ix


def sample_plan(n, d):
    """quant_call_sample (csrc/hdb_ws.h) for rows of up to 512 elements -> (s_tiles, stride); the tests check it against the
    sample_rows statistic of the call"""
    assert d <= 512
    s_tiles = (max(int(16.0 * n / 512.0), 256) + 15) // 16
    s_tiles = max(1, min(s_tiles, n // 16))
    return s_tiles, max(1, (n // 16) // s_tiles)


def sampled_rows(n, d):
    s_tiles, stride = sample_plan(n, d)
    tiles = np.array([tile_index(w, stride) for w in range(s_tiles)], np.int64)
    assert len(set(tiles.tolist())) == s_tiles and tiles.max() < n // 16
    return (tiles[:, None] * 16 + np.arange(16)[None, :]).reshape(-1)


def _three(ix, Q, k, metric, what, n=None, d=None):
    """use_plane = 1, use_plane = 0, use_quant = 0 on one call -> (answer of the plane call, status, plane_survivors, quant_cands)"""
    on = _raw(ix, Q, k, metric)
    assert ix.stat("quant") == 1 and ix.stat("plane") == 1, f"{what}: the call did not take the path"
    if n is not None:
        assert ix.stat("sample_rows") == 16 * sample_plan(n, d)[0], f"{what}: the sample plan is restated wrongly"
    cands_on, surv = ix.stat("quant_cands"), ix.stat("plane_survivors")
    on_h = _host(ix, Q, k, metric)
    ix.set_option("use_plane", 0)
    try:
        off = _raw(ix, Q, k, metric)
        assert ix.stat("quant") == 1 and ix.stat("plane") == 0 and ix.stat("plane_survivors") == 0, what
        cands_off = ix.stat("quant_cands")
        off_h = _host(ix, Q, k, metric)
    finally:
        ix.set_option("use_plane", 1)
    ix.set_option("use_quant", 0)
    try:
        ref = _raw(ix, Q, k, metric)
        assert ix.stat("quant") == 0 and ix.stat("plane") == 0, what
        ref_h = _host(ix, Q, k, metric)
    finally:
        ix.set_option("use_quant", 1)
    print(f"{what}: survivors {surv}, candidates {cands_on} / {cands_off}, status {on[2]} / {off[2]} / {ref[2]}")
    assert cands_on == cands_off, f"{what}: {cands_on} candidates behind the plane, {cands_off} without it"
    assert surv >= cands_on, f"{what}: {surv} survivors, {cands_on} candidates"
    assert np.array_equal(on[2], off[2]), f"{what}: status {on[2]} behind the plane, {off[2]} without it"
    if (on[2] == 0).all():          # (a non-zero status: the device buffers hold a failed attempt's list, the host entry re-runs the call)
        for a, b in zip(on, off):
            assert np.array_equal(a, b), f"{what}: plane on and off differ"
        if (ref[2] == 0).all():
            for a, b in zip(on, ref):
                assert np.array_equal(a, b), f"{what}: differs from the call without the shadow"
    for a, b, c in zip(on_h, off_h, ref_h):
        assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: host answers differ"
    return on, on[2], surv, cands_on


SHAPES = [(8193, 384, "auto"), (8217, 384, "auto"), (70001, 384, "auto"), (70001, 200, "explicit")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,flavour", SHAPES, ids=[f"n{n}-d{d}-{fl}" for n, d, fl in SHAPES])
def test_settings_agree(n, d, flavour):
    """dot and cosine, plain / bias / a mask that keeps 37 rows / a mask that removes every sampled row"""
    torch = _torch()
    ix = _index(_matrix(n, d, seed=3 * n + d), flavour)
    try:
        g = torch.Generator(device="cuda").manual_seed(n + d)
        bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
        few = torch.zeros(n, dtype=torch.uint8, device="cuda")
        few[torch.randperm(n, generator=g, device="cuda")[:37]] = 1
        unsampled = np.ones(n, np.uint8)
        unsampled[sampled_rows(n, d)] = 0
        for mi, metric in enumerate(METRICS):
            Q = np.random.default_rng(n + d + mi).standard_normal((1, d)).astype(np.float32)
            for variant in ("plain", "bias", "few", "unsampled"):
                ix.set_bias((bias * 20.0 if metric == "dot_product" else bias) if variant == "bias" else None)
                ix.set_row_mask(few if variant == "few" else unsampled if variant == "unsampled" else None)
                what = f"n={n} d={d} {flavour} {metric} {variant}"
                ans, st, surv, cands = _three(ix, Q, 100, metric, what, n, d)
                if variant == "few":
                    assert surv <= 37 and cands <= 37
                elif variant == "unsampled":
                    # no sampled row is live: T_s = -inf, every live row is a candidate and no masked row is queued
                    live = int(unsampled.sum())
                    assert surv == live and cands == live, f"{what}: {live} live rows"
                    if live <= 8192:
                        assert (st == 0).all() and unsampled[ans[0][0]].all()
                else:
                    assert (st == 0).all(), f"{what}: status {st}"
                ix.set_bias(None)
                ix.set_row_mask(None)
    finally:
        ix.close()


def _planted(n, d, rows, seed):
    """Gaussian rows; `rows` are the query plus N(0, 1e-3) noise"""
    torch = _torch()
    V = _matrix(n, d, seed)
    q = np.random.default_rng(seed).standard_normal((1, d)).astype(np.float32)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    qt = torch.from_numpy(q).to("cuda")
    V[torch.from_numpy(np.asarray(rows, np.int64)).to("cuda")] = (qt + 1e-3 * torch.randn((len(rows), d), generator=g, device="cuda")).to(torch.float16)
    return V, q


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,flavour", [(70001, 384, "auto"), (8217, 384, "auto"), (70001, 200, "explicit")], ids=("n70001-d384", "n8217-d384", "n70001-d200"))
def test_winners_only_in_sampled_tiles(n, d, flavour):
    """12 near-copies of the query spread over sampled tiles, k = 10: the plane pass never streams those tiles, so the answer comes
    through the list of the sample pass alone."""
    sr = sampled_rows(n, d)
    pick = sr[np.random.default_rng(n).choice(len(sr), 12, replace=False)]
    V, q = _planted(n, d, pick, seed=n + d)
    ix = _index(V, flavour)
    try:
        for metric in METRICS:
            ans, st, surv, cands = _three(ix, q, 10, metric, f"sampled winners n={n} d={d} {metric}", n, d)
            assert (st == 0).all()
            assert set(ans[0][0].tolist()) <= set(pick.tolist()), f"{metric}: {ans[0][0]} are not all planted rows"
            assert cands >= 12
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", (8217, 70001))
def test_winners_only_in_the_ragged_last_tile(n):
    """the last tile (9 rows of 8217, 1 row of 70001) is in no window of the sample: the walk's tail reaches it"""
    d = 384
    last = np.arange((n // 16) * 16, n)
    assert not set(last.tolist()) & set(sampled_rows(n, d).tolist())
    k = min(5, len(last))
    V, q = _planted(n, d, last, seed=n)
    ix = _index(V)
    try:
        for metric in METRICS:
            ans, st, surv, cands = _three(ix, q, k, metric, f"ragged winners n={n} {metric}", n, d)
            assert (st == 0).all()
            assert set(ans[0][0].tolist()) <= set(last.tolist())
    finally:
        ix.close()


@pytest.mark.gpu
def test_list_chunks_refill_full_queues():
    """tests/test_quant_inpass.py's near-copies matrix: 6000 rows that all reach the threshold, sampled ones included, then 2300 far
    below it -- every chunk of the list appends to a queue and drains full tiles."""
    torch = _torch()
    n_near, n_far, d = 6000, 2300, 384
    n = n_near + n_far
    g = torch.Generator(device="cuda").manual_seed(5)
    base = torch.randn((1, d), generator=g, device="cuda", dtype=torch.float32)
    sign = torch.ones((n, 1), device="cuda", dtype=torch.float32)
    sign[n_near:] = -1.0
    V = (sign * base + 1e-3 * torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32)).to(torch.float16)
    q = base.cpu().numpy().astype(np.float32)
    near_sampled = int((sampled_rows(n, d) < n_near).sum())
    assert near_sampled >= 64
    ix = _index(V)
    try:
        for metric in METRICS:
            ans, st, surv, cands = _three(ix, q, 100, metric, f"near copies {metric}", n, d)
            assert (st == 0).all()
            assert n_near <= surv <= n and n_near <= cands <= 8192
    finally:
        ix.close()


def _fold_n(d):
    """the smallest n at which plan_quant folds the threshold into the passes: nsub = 4 x ceil(s_tiles / 4) >= 1024 (hdb_plan.h)"""
    lo, hi = 8193, 1 << 22                       # (s_tiles is non-decreasing in n)
    while lo < hi:
        mid = (lo + hi) // 2
        if (sample_plan(mid, d)[0] + 3) // 4 >= 256:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.gpu
def test_folded_threshold():
    d = 128
    n = _fold_n(d)
    assert 500000 < n < 560000 and (sample_plan(n - 1, d)[0] + 3) // 4 == 255
    sr = sampled_rows(n, d)
    pick = sr[np.random.default_rng(7).choice(len(sr), 12, replace=False)]
    V, q = _planted(n, d, pick, seed=n % 1000)
    ix = _index(V)
    try:
        rng = np.random.default_rng(n % 1000 + 17)          # (not the planted query's seed)
        for metric in METRICS:
            # Gaussian query: ~ 512 rows above the threshold, some of them sampled
            Q = rng.standard_normal((1, d)).astype(np.float32)
            ans, st, surv, cands = _three(ix, Q, 100, metric, f"folded n={n} {metric}", n, d)
            assert (st == 0).all()
            # the planted query: the 10 best are sampled rows
            ans, st, surv, cands = _three(ix, q, 10, metric, f"folded n={n} {metric} planted", n, d)
            assert (st == 0).all() and set(ans[0][0].tolist()) <= set(pick.tolist())
            # the test entry evaluates every tile, sampled ones included
            hi, hi5 = ix.quant_bounds(q[0], M[metric])
            assert hi.shape == (n,) and not np.isnan(hi5).any() and np.isfinite(hi5).all()
            assert (hi5 >= hi).all(), f"hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
    finally:
        ix.close()
