"""The pending queue between the two stages of the plane pass, on the GPU (hdb_quant.hip, "Stage A"; option use_plane: 3 takes the
pass with stage A at every size, 2 the one-stage pass, 0 no plane).

Stage A appends the rows its four-bit bound keeps to a wave-private queue with their terms (row, S4, k_hi and rc codes, the tile's E*,
T*, F*, the bias); stage B takes 16 of them at a time as one virtual tile of bit words, and what is pending after the walk as a ragged
tile.  What must hold on every call: use_plane 0, 2 and 3 give the same indices, score bits, status (0: the contents are chosen so that
no list passes HDB_CAND_CAP = 8192) and quant_cands; plane_survivors with stage A is at most that without it; plane = 1 from 8193
rows on.

Shapes: n in {8193, 8209, 70001} (a ragged last tile of one row each; 8193 is the smallest size that takes the shadow), d in {40, 256,
384, 512}: J = 1 .. 4; the explicit int8 shadow (use_mfma = 0, use_fused = 0) and the automatic fp16 one at d >= 256; dot and cosine;
k = 100.  Contents, each aimed at one way the queue can go wrong:
  dense    200 scaled copies of the query in consecutive rows: stage A keeps all 32 rows of a step, two flushes a step and drains
           inside a flush; once more with max_blocks = 1, four waves walking everything;
  sparse   one near-copy of the query every 37 rows among Gaussian rows scaled by 1e-3: entries wait across many steps and drains;
  ragged   near-copies only in the last full tile and the ragged tile behind it: the end-of-walk flush;
  carried  the heterogeneous tiles of test_plane_block.py with 64 near-copies, a per-row bias from set_recency and a row mask over
           half the copies: the entry's terms and bias, and no masked row ever queued (none is returned);
  nothing  d = 40 only: the query lives in eight dimensions where every streamed row is zero, and the rows that score -- 128 equal
           copies of the query -- lie in sampled tiles, which the pass takes from the sample list: no step keeps a row, the queue stays
           empty to the end and plane_survivors is at most 128.
The counts were read from a GPU run of this file (every call prints its own), not worked out with the numpy models of
test_quant_plane_model.py: the largest quant_cands of any case by content is dense 2681, sparse 1892 (the near-copies), ragged 2888,
carried 2434, nothing 128 -- all below 8192 -- with up to 25312 plane_survivors; every status word is asserted zero.
"""
import numpy as np
import pytest

from test_plane_bit import _call, _index
from test_plane_block import _heterogeneous
from test_plane_skip import sampled_rows

ROWS = (8193, 8209, 70001)
DIMS = (40, 256, 384, 512)                  # U = 2, 8, 12, 16: J = 1, 2, 3, 4
METRICS = ("dot_product", "cosine_similarity")
CAP = 8192
CASES = [(n, d, dt) for n in ROWS for d in DIMS for dt in ("f16", "f16auto") if dt == "f16" or d >= 256]


def _near(q, m, rng, lo=0.97, hi=1.0):
    """m near-copies of q: scales in [lo, hi] and 1 % noise, so scores and cosines are distinct and close to the top"""
    s = rng.uniform(lo, hi, size=(m, 1)).astype(np.float32)
    return s * q[None, :] + (0.01 * rng.standard_normal((m, q.size))).astype(np.float32)


def _small(n, d, rng):
    return (1e-3 * rng.standard_normal((n, d))).astype(np.float32)


def _contents(kind, n, d, q, rng):
    """-> (rows float32, planted row numbers)"""
    if kind == "dense":
        V = _small(n, d, rng)
        rows = 1000 + np.arange(200)
        V[rows] = np.linspace(0.9, 0.5, 200, dtype=np.float32)[:, None] * q[None, :]
    elif kind == "sparse":
        V = _small(n, d, rng)
        rows = np.arange(5, n, 37)
        V[rows] = _near(q, rows.size, rng)
    elif kind == "ragged":
        V = _small(n, d, rng)
        rows = np.arange((n - 1) // 16 * 16 - 16, n)            # the last full tile and the ragged one
        V[rows] = _near(q, rows.size, rng)
    elif kind == "carried":
        V = _heterogeneous(n, d, "f32", seed=n + d)
        rows = np.sort(rng.choice(n - 1, 64, replace=False))
        V[rows] = _near(q, 64, rng, 0.5, 1.0)
    else:                                                        # nothing: see the module's docstring
        assert kind == "nothing" and d == 40
        V = _small(n, d, rng) * 1e3
        V[:, :8] = 0.0
        rows = sampled_rows(n, d)[:128]
        V[rows] = q[None, :]                                     # (equal rows: the threshold, taken inside the sample, is met by all 128)
    return V, rows


def _agree(ix, q, metric, n, what):
    """use_plane 0, 2, 3 on one call -> (indices, survivors with stage A)"""
    (o0, s0, _), (o2, s2, _), (o3, s3, _) = (_call(ix, q[None, :], 100, metric, up) for up in (0, 2, 3))
    print(f"{what}: plane_survivors {s3[2]} with stage A, {s2[2]} without, quant_cands {s3[3]}")
    assert (o0[2] == 0).all() and (o2[2] == 0).all() and (o3[2] == 0).all(), f"{what}: status {o0[2]}, {o2[2]}, {o3[2]}"
    assert s0[0] == s2[0] == s3[0] == 1 and s0[1] == 0 and s2[1] == 1 and s3[1] == 1, f"{what}: quant, plane = {s0[:2]}, {s2[:2]}, {s3[:2]}"
    assert s0[3] == s2[3] == s3[3] <= CAP, f"{what}: quant_cands {s0[3]}, {s2[3]}, {s3[3]}"
    assert s3[2] <= s2[2], f"{what}: {s3[2]} survivors with stage A, {s2[2]} without"
    for a, b, c in zip(o0[:2], o2[:2], o3[:2]):
        assert np.array_equal(a, b) and np.array_equal(a, c), f"{what}: the three settings differ"
    return o3[0][0], s3[2]


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,dt", CASES, ids=[f"n{n}-d{d}-{dt}" for n, d, dt in CASES])
def test_queue(n, d, dt):
    import torch
    assert n > CAP
    for kind in ("dense", "sparse", "ragged", "carried") + (("nothing",) if d == 40 else ()):
        rng = np.random.default_rng(1000 * d + n % 1000 + len(kind))
        q = rng.standard_normal(d).astype(np.float32)
        if kind == "nothing":
            q[8:] = 0.0
        V, rows = _contents(kind, n, d, q, rng)
        ix = _index(V, dt)
        try:
            for metric in METRICS:
                what = f"n={n} d={d} {dt} {kind} {metric}"
                if kind == "carried":
                    scale = float(q @ q) if metric == "dot_product" else 1.0
                    ix.set_recency(rng.uniform(0.0, 5.0, size=n), 0.05 * scale)
                    mask = np.ones(n, np.uint8)
                    mask[rows[::2]] = 0
                    ix.set_row_mask(torch.from_numpy(mask).cuda())
                top, surv = _agree(ix, q, metric, n, what)
                if kind == "carried":
                    assert not np.isin(top, rows[::2]).any(), f"{what}: a masked row came back"
                    if metric == "cosine_similarity":        # (by dot product the tiles' rows of norm up to 1e4 and of +-65504 outrank them)
                        assert np.isin(rows[1::2], top).all(), f"{what}: a near-copy that is not masked is missing"
                    ix.set_bias(None)
                    ix.set_row_mask(None)
                elif kind in ("dense", "nothing"):
                    assert np.isin(top, rows).all(), f"{what}: a row that is no copy came back"
                    assert kind == "dense" or surv <= rows.size, f"{what}: {surv} survivors, but only the {rows.size} sampled copies score"
                elif kind == "ragged":
                    assert np.isin(rows, top).all(), f"{what}: a row of the last two tiles is missing"
                else:
                    assert np.isin(top, rows).all(), f"{what}: a row that is no near-copy came back"
                if kind == "dense":
                    ix.set_option("max_blocks", 1)
                    try:
                        top1, surv1 = _agree(ix, q, metric, n, what + " max_blocks=1")
                    finally:
                        ix.set_option("max_blocks", 0)
                    assert np.array_equal(top, top1) and surv == surv1, f"{what}: one workgroup gives {surv1} survivors, the grid {surv}"
        finally:
            ix.close()
