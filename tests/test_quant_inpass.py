"""The one-query shadow call after its launches were folded (hdb_quant.hip): the pass over the 5-bit plane finishes the rows it keeps
itself, 16 at a time through MODE 1's own evaluation; the kernel that emits a candidate copies its row into the compact matrix of the
matrix-core rescoring.  (Selecting the threshold once, in the sample pass, was measured and not kept -- DESIGN.md; the shapes at
which the threshold is folded into the passes, and the one just below, are checked here all the same.)

The promise is the one tests/test_quant_plane.py checks: indices, score bits and status of a call behind the plane are those of the
call with use_plane = 0, which are those of the call without the shadow; the candidate count is the same with and without the plane.

Shapes.  hdb_topk takes the shadow only for matrices of more than HDB_CAND_CAP = 8192 rows (hdb_plan.h: a "small" matrix goes to the
small path whatever quant_min_n says, and k = 100 needs n >= 3200), so the smallest shapes here stand just above that: 8193 rows (513
tiles: the last step of the plane pass has one tile, of one row) and 8217 rows instead of matrices of a few dozen rows, and 8300 rows
of which 6000 are near-copies of one vector instead of a 6000-row matrix.  A mask that keeps 37 rows gives the call in which no wave
ever holds 16 rows and only the remainder drain works.  d = 200 has no matrix-core geometry of its own, so a one-query fp16 call
there never builds the automatic shadow: that width runs the explicit shadow (VALU bits), as tests/test_quant_plane.py does for such
widths; 128, 384 and 512 run the automatic one (matrix-core bits, the row copies).
"""
import numpy as np
import pytest

from hyperdb import _native

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
K = 100


def _torch():
    import torch
    return torch


def _matrix(n, d, seed):
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn((n, d), generator=g, device="cuda", dtype=torch.float32).to(torch.float16)


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _raw(ix, Q, metric):
    idx, sc, st = ix.topk_device(Q, K, M[metric])
    return idx.cpu().numpy(), _bits(sc.cpu().numpy()), st.cpu().numpy()


def _host(ix, Q, metric):
    idx, sc = ix.topk(Q, K, M[metric])
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


class _Options:
    def __init__(self, ix, **opts):
        self.ix, self.opts = ix, opts

    def __enter__(self):
        for name, v in self.opts.items():
            self.ix.set_option(name, v)

    def __exit__(self, *exc):
        for name in self.opts:
            self.ix.set_option(name, 1)


def _three_settings(ix, Q, metric, what, plane=True, ref_ok=False):
    """use_plane = 1, use_plane = 0, use_quant = 0 on one call.  -> (status of the shadow call, plane_survivors, quant_cands)
    ref_ok: the call without the shadow must itself end with status 0 (Gaussian rows), so that the comparison with it is made."""
    on = _raw(ix, Q, metric)
    assert ix.stat("quant") == 1 and ix.stat("plane") == (1 if plane else 0), f"{what}: the call did not take the path"
    cands_on, surv = ix.stat("quant_cands"), ix.stat("plane_survivors")
    on_h = _host(ix, Q, metric)
    with _Options(ix, use_plane=0):
        off = _raw(ix, Q, metric)
        assert ix.stat("quant") == 1 and ix.stat("plane") == 0 and ix.stat("plane_survivors") == 0, what
        cands_off = ix.stat("quant_cands")
        off_h = _host(ix, Q, metric)
    with _Options(ix, use_quant=0):
        ref = _raw(ix, Q, metric)
        assert ix.stat("quant") == 0 and ix.stat("plane") == 0, what
        ref_h = _host(ix, Q, metric)
    assert not ref_ok or (ref[2] == 0).all(), f"{what}: the call without the shadow ended with status {ref[2]}"
    print(f"{what}: survivors {surv}, candidates {cands_on} / {cands_off}, status {on[2]} / {off[2]} / {ref[2]}")
    assert cands_on == cands_off, f"{what}: {cands_on} candidates behind the plane, {cands_off} without it"
    if plane:
        assert surv >= cands_on, f"{what}: {surv} survivors, {cands_on} candidates"
    assert np.array_equal(on[2], off[2]), f"{what}: status {on[2]} behind the plane, {off[2]} without it"
    # (a non-zero status says that the device buffers hold a failed attempt's partial list, which is each path's own; on rows that
    #  are near-copies of one another the call without the shadow may be the one whose list overflows: its host entry re-runs it)
    if (on[2] == 0).all():
        for a, b in zip(on, off):
            assert np.array_equal(a, b), f"{what}: plane on and off differ"
        if (ref[2] == 0).all():
            for a, b in zip(on, ref):
                assert np.array_equal(a, b), f"{what}: differs from the call without the shadow"
    for a, b, c in zip(on_h, off_h, ref_h):
        assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: host answers differ"
    return on[2], surv, cands_on


def _variants(ix, n, d, seed, what, flavour="auto"):
    """dot and cosine, plain / bias / a mask that keeps 37 rows (fewer than k: the status is HDB_Q_UNDERFLOW on every path)"""
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    bias = (torch.rand(n, generator=g, device="cuda") * 0.05).to(torch.float32)
    few = torch.zeros(n, dtype=torch.uint8, device="cuda")
    few[torch.randperm(n, generator=g, device="cuda")[:37]] = 1
    for mi, metric in enumerate(METRICS):
        Q = np.random.default_rng(seed + mi).standard_normal((1, d)).astype(np.float32)
        for variant in ("plain", "bias", "mask"):
            ix.set_bias((bias * 20.0 if metric == "dot_product" else bias) if variant == "bias" else None)
            ix.set_row_mask(few if variant == "mask" else None)
            st, surv, cands = _three_settings(ix, Q, metric, f"{what} {metric} {variant}", ref_ok=variant != "mask")
            if variant == "mask":
                assert surv <= 37 and cands <= 37
            else:
                assert (st == 0).all(), f"{what} {metric} {variant}: status {st}"
            ix.set_bias(None)
            ix.set_row_mask(None)


# J = ceil(U / 4) plane pieces per lane: d = 128 -> 1, 200 -> 2 (7 units: an odd count), 384 -> 3, 512 -> 4
SHAPES = [(70001, 128, "auto"), (70001, 200, "explicit"), (70001, 384, "auto"), (70001, 512, "auto"),
          (8193, 384, "auto"), (8217, 384, "auto")]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,flavour", SHAPES, ids=[f"n{n}-d{d}-{fl}" for n, d, fl in SHAPES])
def test_ragged_ends_and_every_width(n, d, flavour):
    ix = _index(_matrix(n, d, seed=n + d), flavour)
    try:
        _variants(ix, n, d, n + d, f"n={n} d={d} {flavour}", flavour)
    finally:
        ix.close()


def _near_copies(n_near, n_far, d, seed):
    """n_near rows that are one random vector plus N(0, 1e-3) noise, then n_far rows that are its negative plus the same noise: for a
    query along the vector every near row reaches the threshold and no far row does."""
    torch = _torch()
    g = torch.Generator(device="cuda").manual_seed(seed)
    base = torch.randn((1, d), generator=g, device="cuda", dtype=torch.float32)
    sign = torch.ones((n_near + n_far, 1), device="cuda", dtype=torch.float32)
    sign[n_near:] = -1.0
    V = sign * base + 1e-3 * torch.randn((n_near + n_far, d), generator=g, device="cuda", dtype=torch.float32)
    return V.to(torch.float16), base.cpu().numpy().astype(np.float32)


@pytest.mark.gpu
def test_every_row_survives_and_the_candidates_fit():
    """6000 near-copies (and 2300 rows far below them, so that the matrix is large enough for the path): the queue of every wave
    refills on every step, full tiles and the ragged one alternate, and workgroups fill their stage (128 entries) to the brim."""
    n_near, n_far, d = 6000, 2300, 384
    n = n_near + n_far
    V, q = _near_copies(n_near, n_far, d, seed=5)
    ix = _index(V)
    try:
        for metric in METRICS:
            st, surv, cands = _three_settings(ix, q, metric, f"near copies {metric}")
            assert (st == 0).all()
            assert n_near <= surv <= n and surv >= n // 2
            assert n_near <= cands <= 8192
    finally:
        ix.close()


@pytest.mark.gpu
def test_every_row_survives_and_the_list_overflows():
    n, d = 20000, 384
    V, q = _near_copies(n, 0, d, seed=6)
    ix = _index(V)
    try:
        for metric in METRICS:
            st, surv, cands = _three_settings(ix, q, metric, f"overflow {metric}")
            assert (st & _native.Q_OVERFLOW).all(), f"status {st}"
            assert surv >= n // 2 and cands > 8192
    finally:
        ix.close()


@pytest.mark.gpu
def test_plane_cap_rows_is_a_statistic():
    n_near, n_far, d = 6000, 2300, 384
    n = n_near + n_far
    V, q = _near_copies(n_near, n_far, d, seed=5)
    ix = _index(V)
    try:
        ix.set_option("plane_cap_rows", n)
        big = _raw(ix, q, "cosine_similarity")
        assert ix.stat("plane") == 1 and ix.stat("plane_overflows") == 0
        surv, cands = ix.stat("plane_survivors"), ix.stat("quant_cands")
        assert 16 < surv <= n
        ix.set_option("plane_cap_rows", 16)
        small = _raw(ix, q, "cosine_similarity")
        assert ix.stat("plane") == 1 and ix.stat("plane_overflows") == 1
        assert ix.stat("plane_survivors") == surv and ix.stat("quant_cands") == cands
        small2 = _raw(ix, q, "cosine_similarity")
        assert ix.stat("plane_overflows") == 2
        for a, b, c in zip(big, small, small2):
            assert np.array_equal(a, b) and np.array_equal(a, c)
        assert (big[2] == 0).all()
    finally:
        ix.close()


# The threshold is folded into the two passes when the sample pass's grid has at least 1024 waves (hdb_plan.h, plan_quant:
# nsub = 4 x workgroups, kept when 1024 <= nsub <= 4096).  For d <= 512 the sample aims at 512 rows (hdb_ws.h, quant_sample_target), so it has
# s_tiles = (max(floor(16 n / 512), 256) + 15) / 16 = (floor(n / 32) + 15) / 16 tiles, four to a workgroup (hdb_quant_scan_blocks:
# ceil(s_tiles / 4), at most 1024).  256 workgroups need s_tiles >= 1021, i.e. floor(n / 32) >= 16321, i.e. n >= 522272; one row
# fewer gives 1020 tiles, 255 workgroups, nsub = 1020 < 1024: hdb_sample_thr_kernel.
N_FOLD = 522272


@pytest.mark.gpu
@pytest.mark.parametrize("n", (N_FOLD, N_FOLD - 1), ids=("folded", "sample-thr-kernel"))
def test_threshold_folded_and_not(n):
    d = 128
    ix = _index(_matrix(n, d, seed=n % 1000))
    try:
        rng = np.random.default_rng(n % 1000)
        Q4 = rng.standard_normal((4, d)).astype(np.float32)
        for metric in METRICS:
            # one query behind the plane, the same with use_plane = 0, and without the shadow
            st, _, _ = _three_settings(ix, Q4[:1], metric, f"n={n} one query {metric}", ref_ok=True)
            assert (st == 0).all()
            # four queries: the dense MODE 1 pass with the same threshold hand-over
            four = _raw(ix, Q4, metric)
            assert ix.stat("quant") == 1 and ix.stat("plane") == 0
            four_h = _host(ix, Q4, metric)
            with _Options(ix, use_quant=0):
                ref = _raw(ix, Q4, metric)
                assert ix.stat("quant") == 0
                ref_h = _host(ix, Q4, metric)
            assert (ref[2] == 0).all() and np.array_equal(four[2], ref[2]), f"status {four[2]} / {ref[2]}"
            for a, b in zip(four, ref):
                assert np.array_equal(a, b), f"n={n} four queries {metric}: differs from the call without the shadow"
            for a, b in zip(four_h, ref_h):
                assert np.array_equal(a, b)
            # the counters of a call are zeroed by its query prep: five calls on one handle, one answer
            first = _raw(ix, Q4[:1], metric)
            assert ix.stat("quant") == 1 and ix.stat("plane") == 1
            cands = ix.stat("quant_cands")
            for _ in range(4):
                again = _raw(ix, Q4[:1], metric)
                assert ix.stat("quant_cands") == cands
                for a, b in zip(first, again):
                    assert np.array_equal(a, b)
    finally:
        ix.close()


@pytest.mark.gpu
def test_plane_bound_covers_the_int8_bound():
    n, d = 70001, 384
    rng = np.random.default_rng(11)
    Vh = rng.standard_normal((n, d)).astype(np.float16)
    bias = (rng.random(n) * 0.05).astype(np.float32)
    mask = (rng.random(n) < 0.5).astype(np.uint8)
    q = rng.standard_normal(d).astype(np.float32)
    ix = _index(Vh)
    try:
        ix.topk_device(q[None, :], 10, M["cosine_similarity"])                       # (the automatic flavour builds its shadow here)
        assert ix.stat("plane") == 1
        for metric in METRICS:
            for variant in ("plain", "bias", "mask"):
                ix.set_bias(bias if variant == "bias" else None)
                ix.set_row_mask(mask if variant == "mask" else None)
                hi, hi5 = ix.quant_bounds(q, M[metric])
                live = mask != 0 if variant == "mask" else np.ones(n, bool)
                assert not np.isnan(hi5).any()
                assert (hi5[live] >= hi[live]).all(), f"{metric} {variant}: hi5 < hi at rows {np.flatnonzero(live & (hi5 < hi))[:8]}"
                if variant == "mask":
                    assert np.isneginf(hi5[~live]).all() and np.isneginf(hi[~live]).all()
                ix.set_bias(None)
                ix.set_row_mask(None)
    finally:
        ix.close()
