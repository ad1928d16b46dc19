"""The plane pass on its hot blocks, on the GPU (hdb_quant.hip, "The 5-bit plane": the hot block; hdb_caps.h, hdb_plane_*).

Pass 1 reads, per 16-row tile and metric, 64 bytes of row terms: every row's scale rounded up to bfloat16, its residual norm as a
byte, and the tile's maxima E*, T*, F*.  What must hold is what held before: hi5 >= hi for every row (hi as MODE 1 computes it),
and the candidate list, indices, score bits and status of a call are those of the call without the plane and without the shadow.
The matrices here are the ones that strain the new terms: tiles whose rows' norms run from 1e-4 to 1e4, all-zero rows and rows of
+-65504 mixed into ordinary tiles, a ragged last tile.  The maxima are tile state, so the plane after an update, an extend into a
ragged tile and a compaction is compared with that of a fresh index over the same rows.
"""
import numpy as np
import pytest

from test_quant_plane import AUTO_DIMS, DIMS, M, METRICS, ROWS, _identity, _index, _raw

CASES = [(d, n, fl, dt) for d in DIMS for n in ROWS for fl, dt in (("auto", "f16"), ("explicit", "f16"), ("explicit", "f32"))
         if fl == "explicit" or d in AUTO_DIMS]


def _heterogeneous(n, d, dt, seed):
    """Ordinary Gaussian rows; in every third tile the rows' norms run from 1e-4 to 1e4; zero rows and rows of +-65504 at random
    places (never a tile of their own: at most two extreme rows in a tile of 16)."""
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((n, d)).astype(np.float32)
    wild = np.flatnonzero((np.arange(n) // 16) % 3 == 1)
    norms = 10.0 ** rng.uniform(-4, 4, size=wild.size)
    V[wild] *= (norms / np.linalg.norm(V[wild].astype(np.float64), axis=1))[:, None].astype(np.float32)
    tiles = rng.permutation(n // 16)[:120]
    slots = rng.integers(0, 16, size=(120, 2))
    for i, t in enumerate(tiles):
        r0, r1 = 16 * t + slots[i]
        kind = i % 3
        V[r0] = 0.0 if kind == 0 else (65504.0 if kind == 1 else -65504.0)
        if r1 != r0:
            V[r1] = np.where(rng.integers(0, 2, size=d) == 1, 65504.0, -65504.0) if kind == 0 else 0.0
    V[n - 1] = 65504.0                               # the ragged last tile holds an extreme row too
    V = np.clip(V, -65504.0, 65504.0)
    return V.astype(np.float16) if dt == "f16" else V.astype(np.float16).astype(np.float32)


_SURVIVORS = {}


@pytest.mark.gpu
@pytest.mark.parametrize("d,n,flavour,dt", CASES, ids=[f"d{d}-n{n}-{fl}-{dt}" for d, n, fl, dt in CASES])
def test_heterogeneous_tiles(d, n, flavour, dt):
    V = _heterogeneous(n, d, dt, seed=7 * d + n)
    rng = np.random.default_rng(d + n)
    queries = [rng.standard_normal(d).astype(np.float32), (rng.standard_normal(d) * 1e-3).astype(np.float32)]
    one = np.zeros(d, np.float32); one[d // 3] = -2.5
    queries.append(one)
    bias = (rng.random(n) * 0.05).astype(np.float32)
    ix = _index(V, flavour)
    try:
        ix.topk_device(queries[0][None, :], 10, M["cosine_similarity"])             # (the automatic flavour builds its shadow here)
        assert ix.stat("plane") == 1
        for metric in METRICS:
            for variant in ("plain", "bias"):
                b = None if variant == "plain" else (bias * 1e6 if metric == "dot_product" else bias)
                ix.set_bias(b)
                for qi, q in enumerate(queries):
                    hi, hi5 = ix.quant_bounds(q, M[metric])
                    what = f"d={d} n={n} {flavour} {dt} {metric} {variant} query {qi}"
                    assert np.isfinite(hi5).all(), f"{what}: hi5 not finite at rows {np.flatnonzero(~np.isfinite(hi5))[:8]}"
                    assert (hi5 >= hi).all(), f"{what}: hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
                surv = _identity(ix, flavour, queries[0][None, :], 100, metric, f"d={d} n={n} {flavour} {dt} {metric} {variant}")
                _SURVIVORS[(d, n, flavour, dt, metric, variant)] = surv
                ix.set_bias(None)
        print(f"plane_survivors d={d} n={n} {flavour} {dt}:", {k[4:]: v for k, v in _SURVIVORS.items() if k[:4] == (d, n, flavour, dt)})
    finally:
        ix.close()


def _same_as_fresh(ix, rows, flavour, q, what):
    for metric in METRICS:
        got = _raw(ix, q, 100, metric)
        assert ix.stat("plane") == 1, what
        surv, cands = ix.stat("plane_survivors"), ix.stat("quant_cands")
        fresh = _index(rows, flavour)
        try:
            want = _raw(fresh, q, 100, metric)
            assert fresh.stat("plane") == 1
            assert surv == fresh.stat("plane_survivors"), f"{what} {metric}: {surv} survivors, a fresh index {fresh.stat('plane_survivors')}"
            assert cands == fresh.stat("quant_cands"), f"{what} {metric}: {cands} candidates, a fresh index {fresh.stat('quant_cands')}"
        finally:
            fresh.close()
        for a, b in zip(got, want):
            assert np.array_equal(a, b), f"{what} {metric}: differs from a fresh index"


def _bounds_as_fresh(ix, rows, flavour, q, what):
    """The tile state itself: hi5 of every row, bit for bit that of a fresh index over the same rows, and at least MODE 1's hi."""
    fresh = _index(rows, flavour)
    try:
        fresh.topk_device(q, 10, M["cosine_similarity"])                            # (the automatic flavour builds its shadow here)
        for metric in METRICS:
            hi, hi5 = ix.quant_bounds(q[0], M[metric])
            _, want5 = fresh.quant_bounds(q[0], M[metric])
            assert (hi5 >= hi).all(), f"{what} {metric}: hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
            diff = np.flatnonzero(hi5.view(np.int32) != want5.view(np.int32))
            assert diff.size == 0, f"{what} {metric}: hi5 differs from a fresh index at rows {diff[:8]}"
    finally:
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ("auto", "explicit"))
def test_tile_state_after_maintenance(flavour):
    rng = np.random.default_rng(31)
    n, d = 8209, 384                                 # 8209 = 16 x 513 + 1: the last tile holds one row
    V = (rng.standard_normal((n + 5, d)) * 0.01).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)
    ix = _index(V[:n].copy(), flavour)
    try:
        _same_as_fresh(ix, V[:n], flavour, q, "fresh")
        # one row of a tile to 1e4 times its neighbours' norm, then back: the tile's maxima follow both ways
        W = V[:n].copy()
        W[4005] = (W[4005].astype(np.float32) * 1e4).astype(np.float16)
        ix.update(W)
        _same_as_fresh(ix, W, flavour, q, "one row of a tile 1e4 times larger")
        ix.update(V[:n].copy())
        _same_as_fresh(ix, V[:n], flavour, q, "the row back to its size")
        # five rows into the ragged last tile, a thousand times the norm of the row that was there
        V[n:] = (V[n:].astype(np.float32) * 1e3).astype(np.float16)
        ix.append(V[n:])
        _same_as_fresh(ix, V, flavour, q, "after an extend into the ragged tile")
        _bounds_as_fresh(ix, V, flavour, q, "after an extend into the ragged tile")
        keep = np.sort(rng.choice(n + 5, 8201, replace=False))     # (more than HDB_CAND_CAP rows stay: the call still takes the shadow)
        keep[-1] = n + 4                             # one of the large rows moves into another tile
        ix.compact(keep)
        _same_as_fresh(ix, V[keep], flavour, q, "after compaction")
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ("auto", "explicit"))
def test_extend_beside_a_large_resident_row(flavour):
    """The only partial derivation there is (hdb_index_update rebuilds every tile): an extend into the ragged last tile.  Here the
    row that is already there is a thousand times larger than the five that arrive, so the tile's E*, T* and F* are decided by the
    resident neighbour: a derivation from the appended rows alone would leave the tile's dot-product maxima a thousand times too
    small and hi5 of the resident row below hi.  And the other way round in the cosine block, where the small rows' 1 / ||v|| sets F*."""
    rng = np.random.default_rng(37)
    n, d = 8209, 384                                 # the last tile holds row 8208 alone
    V = (rng.standard_normal((n + 5, d)) * 0.01).astype(np.float16)
    q = rng.standard_normal((1, d)).astype(np.float32)
    V[n - 1] = (q[0] * 3.0).astype(np.float16)       # large, and aligned with the query: it belongs at the top of a dot-product call
    V[n:] = (V[n:].astype(np.float32) * 0.01).astype(np.float16)
    ix = _index(V[:n].copy(), flavour)
    try:
        _same_as_fresh(ix, V[:n], flavour, q, "fresh")
        ix.append(V[n:])
        _bounds_as_fresh(ix, V, flavour, q, "small rows beside a large resident row")
        _same_as_fresh(ix, V, flavour, q, "small rows beside a large resident row")
        assert n - 1 in _raw(ix, q, 100, "dot_product")[0][0].tolist()
    finally:
        ix.close()
