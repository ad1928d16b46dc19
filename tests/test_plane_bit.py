"""The plane pass in two stages, on the GPU (hdb_quant.hip, "Stage A"; option use_plane: 1 the default, stage A where it was
measured to pay (hdb_caps.h); 2 without stage A; 3 stage A at every size).

Stage A bounds every row from its nibbles and the tile's R4*; only the rows it cannot reject have their bit words read and go through
the five-bit bound, which decides the queue as before.  What must hold: use_plane 0, 1, 2 and 3 give the same indices, score bits, status
and quant_cands on every call; plane_survivors with stage A is at most that without it; and after an append, an update and a
compaction a call gives the survivors and candidates of a fresh index over the same rows (R4* is tile state, derived with E*, T*, F*).

Shapes: n in {16, 17, 8193, 70001} (up to HDB_CAND_CAP rows a call does not take the shadow, so the three settings agree trivially
there and `plane` is asserted from 8193 rows on), d in {16, 40, 256, 384, 512}: J = 1, 1, 2, 3, 4 (256 is added to the widths the issue
lists, which skip J = 2).  Rows: Gaussian; the heterogeneous tiles of
test_plane_block.py; rows whose codes are all +-127; rows whose codes are 16 n - 128 (rho4 = -8) in every element but the one that sets
the scale.  Where the status of a call is not zero (a query that is not finite) the device buffers hold a failed attempt's partial
list, which the host entry discards for the exact re-run: buffers are compared where the status is zero, host answers always.
"""
import numpy as np
import pytest

from hyperdb import _native
from test_plane_block import _heterogeneous

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
ROWS = (16, 17, 8193, 70001)
DIMS = (16, 40, 256, 384, 512)              # U = 1, 2, 8, 12, 16: J = 1, 1, 2, 3, 4
CAP = 8192
CONTENTS = ("gauss", "hetero", "pm127", "rho4")
CASES = [(d, dt) for d in DIMS for dt in ("f16", "f32", "bf16", "f16auto") if dt != "f16auto" or d in (256, 384, 512)]


def _rows(kind, n, d, seed):
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return rng.standard_normal((n, d)).astype(np.float32)
    if kind == "hetero":
        return _heterogeneous(n, d, "f32", seed)
    if kind == "pm127":                              # every code +-127: rows of +-a, a per row
        a = (2.0 ** rng.integers(-6, 7, size=n)).astype(np.float32)
        return np.where(rng.integers(0, 2, size=(n, d)) == 1, 1.0, -1.0).astype(np.float32) * a[:, None]
    V = (16.0 * rng.integers(1, 16, size=(n, d)) - 128.0).astype(np.float32)     # codes 16 m - 128: rho4 = -8
    V[np.arange(n), rng.integers(0, d, size=n)] = 127.0                           # (the scale: s_r = 1, codes are the values)
    return V


def _index(V32, dt):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(V32))
    if dt == "bf16":
        ix = _native.GpuIndex(t.to(torch.bfloat16).cuda())
        ix.set_option("bf16_quant", 1)
        ix.quantize("int8")
    elif dt == "f16auto":
        ix = _native.GpuIndex(t.to(torch.float16).cuda())
    else:
        ix = _native.GpuIndex(t.to(torch.float16 if dt == "f16" else torch.float32).cuda())
        ix.quantize("int8")
        ix.set_option("use_mfma", 0)
        ix.set_option("use_fused", 0)
    ix.set_option("quant_min_n", 0)
    ix.set_option("plane_min_n", 0)
    return ix


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.int32)


def _call(ix, Q, k, metric, use_plane):
    ix.set_option("use_plane", use_plane)
    try:
        idx, sc, st = ix.topk_device(Q, k, M[metric])
        out = (idx.cpu().numpy(), _bits(sc.cpu().numpy()), st.cpu().numpy())
        stats = (ix.stat("quant"), ix.stat("plane"), ix.stat("plane_survivors"), ix.stat("quant_cands"))
        host = None
        if (out[2] != 0).any():
            try:
                hi, hs = ix.topk(Q, k, M[metric])
                host = (np.asarray(hi), _bits(hs))
            except ValueError:                       # (a NaN query: the host entry refuses it, whatever the setting)
                host = (np.zeros(0), np.zeros(0))
        return out, stats, host
    finally:
        ix.set_option("use_plane", 1)


def _three_settings(ix, Q, k, metric, n, what):
    """use_plane 0, 3, 2 and the default on one call -> (plane_survivors with stage A, without it, quant_cands)"""
    (o0, s0, h0), (o1, s1, h1), (o2, s2, h2), (o3, s3, h3) = (_call(ix, Q, k, metric, up) for up in (0, 3, 2, 1))
    # the default is one of the two passes, whichever the size rule picks
    assert s3[1:] in (s1[1:], s2[1:]), f"{what}: the default's plane, survivors, candidates {s3[1:]}"
    assert np.array_equal(o3[2], o0[2]), f"{what}: status of the default {o3[2]}"
    if (o0[2] == 0).all():
        assert np.array_equal(o3[0], o0[0]) and np.array_equal(o3[1], o0[1]), f"{what}: the default differs"
    if n > CAP:
        assert s1[0] == 1 and s1[1] == 1 and s2[1] == 1 and s0[1] == 0, f"{what}: quant, plane = {s0[:2]}, {s1[:2]}, {s2[:2]}"
    print(f"{what}: plane_survivors {s1[2]} with stage A, {s2[2]} without, quant_cands {s1[3]}")
    assert s0[3] == s1[3] == s2[3], f"{what}: quant_cands {s0[3]}, {s1[3]}, {s2[3]}"
    assert s1[2] <= s2[2], f"{what}: {s1[2]} survivors with stage A, {s2[2]} without"
    assert np.array_equal(o0[2], o1[2]) and np.array_equal(o0[2], o2[2]), f"{what}: status {o0[2]}, {o1[2]}, {o2[2]}"
    if (o0[2] == 0).all():
        for a, b, c in zip(o0[:2], o1[:2], o2[:2]):
            assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: the three settings differ"
    else:
        for a, b, c in zip(h0, h1, h2):
            assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: host answers of the three settings differ"
    return s1[2], s2[2], s1[3]


@pytest.mark.gpu
@pytest.mark.parametrize("d,dt", CASES, ids=[f"d{d}-{dt}" for d, dt in CASES])
def test_three_settings(d, dt):
    import torch
    rng = np.random.default_rng(100 + d)
    q = rng.standard_normal(d).astype(np.float32)
    special = {"zero": np.zeros(d, np.float32), "nan": q.copy(), "inf": q.copy()}
    special["nan"][d // 2] = np.nan
    special["inf"][d // 3] = np.inf
    for n in ROWS:
        k = min(100, n)
        bias = (rng.random(n) * 0.05).astype(np.float32)
        mask = torch.from_numpy((rng.random(n) < 0.6).astype(np.uint8)).cuda()
        mask[:k] = 1                                 # (at least k rows stay)
        for kind in CONTENTS:
            ix = _index(_rows(kind, n, d, seed=7 * d + n), dt)
            try:
                for metric in METRICS:
                    for variant in ("plain", "bias", "mask", "bias+mask"):
                        scale = 20.0 if metric == "dot_product" else 1.0
                        ix.set_bias(torch.from_numpy(bias * scale).cuda() if "bias" in variant else None)
                        ix.set_row_mask(mask if "mask" in variant else None)
                        _three_settings(ix, q[None, :], k, metric, n, f"d={d} {dt} n={n} {kind} {metric} {variant}")
                        if variant in ("plain", "bias+mask"):
                            for name, qs in special.items():
                                _three_settings(ix, qs[None, :], k, metric, n, f"d={d} {dt} n={n} {kind} {metric} {variant} {name} query")
                    ix.set_bias(None)
                    ix.set_row_mask(None)
            finally:
                ix.close()


def _same_as_fresh(ix, V32, dt, q, what):
    for metric in METRICS:
        got, stats, _ = _call(ix, q, 100, metric, 3)
        assert stats[1] == 1, f"{what} {metric}: the call did not take the plane"
        fresh = _index(V32, dt)
        try:
            want, fstats, _ = _call(fresh, q, 100, metric, 3)
            _, fstats2, _ = _call(fresh, q, 100, metric, 2)
        finally:
            fresh.close()
        assert stats[2] == fstats[2], f"{what} {metric}: {stats[2]} survivors, a fresh index {fstats[2]}"
        assert stats[3] == fstats[3] == fstats2[3], f"{what} {metric}: {stats[3]} candidates, a fresh index {fstats[3]}"
        assert fstats[2] <= fstats2[2]
        for a, b in zip(got, want):
            assert np.array_equal(a, b), f"{what} {metric}: differs from a fresh index"


def _graded(q, m, d, rng):
    """m rows of codes 16 j - 128 (rho4 = -8 in every element but the one that sets the scale) whose alignment with q rises from none
    to full, so their scores run from the bulk of the matrix to its top and some lie right at the threshold."""
    t = np.linspace(0.0, 1.0, m)[:, None]
    base = t * (q / np.abs(q).max()) * 112.0 + (1.0 - t) * rng.uniform(-112.0, 112.0, size=(m, d))
    V = np.clip(16.0 * np.round(base / 16.0), -112.0, 112.0).astype(np.float32)
    V[np.arange(m), rng.integers(0, d, size=m)] = 127.0
    return V * np.float32(2.0 ** -12)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ("f16", "f16auto"))
def test_r4_after_maintenance(dt):
    """R4* follows its tile.  Rows of rho4 = -8 codes (the largest ||rho4|| there is) arrive in tiles of Gaussian rows by update, sit in
    the ragged last tile when small rows are appended beside them, and move by a compaction.  The query has a constant offset, so
    sum c_q is far from zero and C - C4 = -8 sum c_q is as large as it gets: the four-bit centre under-estimates these rows most, and
    a tile whose R4* were its Gaussian rows' would drop those of them whose score lies just above the threshold -- quant_cands would
    fall below that of the one-stage pass, which _same_as_fresh compares."""
    rng = np.random.default_rng(41)
    n, d = 8209, 384                                 # 8209 = 16 x 513 + 1: the last tile holds one row
    V = (rng.standard_normal((n + 5, d)) * 0.01).astype(np.float16).astype(np.float32)
    q = (rng.standard_normal((1, d)) - 1.0).astype(np.float32)
    wide = _graded(q[0], 300, d, rng)

    def dev(a):
        return np.ascontiguousarray(a).astype(np.float16)

    ix = _index(V[:n].copy(), dt)
    try:
        _same_as_fresh(ix, V[:n], dt, q, "fresh")
        W = V[:n].copy()
        W[16 * np.arange(100, 400) + 5] = wide       # one per tile, 300 tiles
        W[n - 1] = wide[150]                         # ... and the resident row of the ragged tile
        ix.update(dev(W))
        _same_as_fresh(ix, W, dt, q, "rho4 = -8 rows into 300 tiles")
        top = _call(ix, q, 100, "dot_product", 3)[0][0][0]
        assert (((top % 16) == 5) & (top >= 1600) & (top < 6400)).sum() >= 50, "the graded rows do not reach the top of the ranking"
        W = np.concatenate([W, V[n:]])               # five small rows beside the large resident row
        ix.append(dev(V[n:]))
        _same_as_fresh(ix, W, dt, q, "after an extend into the ragged tile")
        keep = np.sort(rng.choice(n + 5, 8201, replace=False))     # (more than HDB_CAND_CAP rows stay: the call still takes the shadow)
        keep[-1] = n + 4
        ix.compact(keep)
        _same_as_fresh(ix, W[keep], dt, q, "after compaction")
        ix.update(dev(V[:n]))
        _same_as_fresh(ix, V[:n], dt, q, "the rows back")
    finally:
        ix.close()
