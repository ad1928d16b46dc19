"""GPU tests (-m gpu) of large MXFP4 batches on the bf16 matrix cores with the query parts in LDS (csrc/hdb_mfma_f4_lds.h): the opt-in
set_option("f8_lds_min_q", n) beside set_option("b1_mfma_min_q", n) on a storage="mxfp4" index.  Two references: the register
flavour (csrc/hdb_mfma_f4.h, the same call with f8_lds_min_q = 0), which walks K in the same order -- indices, score bits and status
are EQUAL -- and oracle/ranking_oracle.py, plain float64 numpy, at the project's 1e-5 * max(1, |s|).  Inputs, N (525 tiles: an odd
count, a ragged last tile) and k as tests/test_mxf4_mfma.py."""
import numpy as np
import pytest
from oracle import ranking_oracle as orc
from test_mxf4_mfma import K, MM_METRICS, N, TOL, _index

pytestmark = pytest.mark.gpu
COS = "cosine_similarity"


def _call(ix, Q, metric, lds, mfma=1, exact=False):
    from hyperdb._native import METRIC_IDS
    out = [t.cpu().numpy() for t in ix.topk_device(Q, K, METRIC_IDS[metric], exact=exact)]
    assert ix.stat("f8_lds") == lds and ix.stat("mfma") == mfma, (metric, Q.shape, exact)
    return out


@pytest.mark.parametrize("nq", [5, 49, 65])
@pytest.mark.parametrize("d", [128, 256, 384, 512])
def test_parity(d, nq):
    """One partial group; a second grid row of one query at d = 512 (three groups per workgroup) and a partial fourth group elsewhere;
    two grid rows at four groups.  Every metric with and without a bias, sampled (MODE 0 + MODE 1) and once per width exact; query 0 is
    stored row N - 2, which the euclidean re-score puts first."""
    ix, _, _, W = _index(d)
    rng = np.random.default_rng(37 * d + nq)
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[0] = W[N - 2]
    bias = rng.uniform(-0.05, 0.05, N).astype(np.float32)
    try:
        ix.set_option("b1_mfma_min_q", 5)
        for b in (None, bias):
            ix.set_bias(b)
            for metric in MM_METRICS:
                for exact in ((False, True) if (nq == 5 and metric == COS) else (False,)):
                    ix.set_option("f8_lds_min_q", 5)
                    gi, gs, st = _call(ix, Q, metric, 1, exact=exact)
                    ix.set_option("f8_lds_min_q", 0)
                    ri, rs, rst = _call(ix, Q, metric, 0, exact=exact)
                    assert (st == 0).all(), (metric, exact, st)
                    assert gi.tobytes() == ri.tobytes() and gs.tobytes() == rs.tobytes() and st.tobytes() == rst.tobytes(), (metric, exact, b is None)
                    for qi in (0, nq - 1):
                        orc.check_topk(gi[qi], gs[qi], W, Q[qi], metric, K, bias=None if b is None else b.astype(np.float64), tol=TOL)
                    if metric == "euclidean_metric":
                        assert gi[0][0] == N - 2 and gs[0][0] == np.float32(1.0) + (0 if b is None else b[N - 2])
    finally:
        ix.close()


def test_what_keeps_its_path():
    """f8_lds_min_q alone, 4 queries, manhattan, d = 544, wide rows (d = 768 under f8_ks_min_q), use_mfma = 0, a matrix with one
    overflowing block (scale byte 254, code 6) and f8_lds_min_q = -1: stat("f8_lds") stays 0 and indices, score bits and status are
    those of the same call with the option at 0."""
    from hyperdb._native import GpuIndex
    ix, c, s, _ = _index(384)
    odd, wide = _index(544)[0], _index(768)[0]
    c2, s2 = c.copy(), s.copy()
    c2[100, 48:64], s2[100, 3] = 0x66, 254
    inf = GpuIndex((c2, s2), storage="mxfp4")
    rng = np.random.default_rng(4)
    Q, Q544, Q768 = (rng.standard_normal((16, d)).astype(np.float32) for d in (384, 544, 768))
    # (handle, queries, metric, other options, f8_lds_min_q, the call's stat("mfma"))
    cases = [(ix, Q, COS, {"b1_mfma_min_q": 0}, 5, 0), (ix, Q[:4], COS, {}, 5, 0), (ix, Q, "manhattan_distance", {}, 5, 0), (odd, Q544, COS, {}, 5, 0),
             (wide, Q768, COS, {"f8_ks_min_q": 5}, 5, 1), (ix, Q, COS, {"use_mfma": 0}, 5, 0), (inf, Q, COS, {}, 5, 0), (ix, Q, COS, {}, -1, 1)]
    try:
        for h, q, metric, opts, value, mfma in cases:
            for name, v in {"b1_mfma_min_q": 5, **opts}.items():
                h.set_option(name, v)
            got = []
            for option in (value, 0):
                h.set_option("f8_lds_min_q", option)
                got.append(_call(h, q, metric, 0, mfma))
            for name in opts:
                h.set_option(name, 1 if name == "use_mfma" else 0)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(*got)), (metric, q.shape, opts, value)
        ix.set_option("b1_mfma_min_q", 5)
        ix.set_option("f8_lds_min_q", 5)
        _call(ix, Q, COS, 1)                              # (the same handle and queries do take the flavour once nothing holds them back)
    finally:
        for h in (ix, odd, wide, inf):
            h.close()


@pytest.mark.parametrize("b1, lds, reads", [(0, 0, 0), (5, 0, 0), (0, 5, 0), (5, 3, 5), (5, 16, 16), (5, -1, 0), (-1, 5, 0)])
def test_the_threshold_in_force(b1, lds, reads):
    ix, wide = _index(256)[0], _index(768)[0]
    try:
        for h in (ix, wide):
            h.set_option("b1_mfma_min_q", b1)
            h.set_option("f8_lds_min_q", lds)
            h.set_option("f8_ks_min_q", 5)
        assert ix.stat("f8_lds_min_q") == reads and wide.stat("f8_lds_min_q") == 0
    finally:
        ix.close()
        wide.close()
