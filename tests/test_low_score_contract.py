"""GPU tests (-m gpu) of the score contract where the rest of the suite never looks: float32 rows whose dot product is small against
|v| |q| (tests/lowscore.py; the inputs' own conditions are checked on the CPU by tests/test_low_score_inputs.py), and three edges
of the dispatch: an infinite row element on a padded width, an infinite query element on the exact path, a manhattan difference
beyond fp16 range.

The contract: |got - exact| <= 1e-5 * max(1, |s|) against the float64-exact score of the stored values (oracle.check_topk; 1e-3 on
fp16 data).  Every matrix has 20 005 rows: above HDB_CAND_CAP, so no call is "small", with a ragged last tile of every tile height.

On the parent of the change that added this module (float32 dot_product batches multiplied as bf16 parts) the dot_product cases
failed with score errors of up to 2.3 bands (a row outside the band in 16 of 16 queries at d = 384), the infinite-row cases of the
padded float32 / fp16 MFMA flavours returned NaN -> -inf, hdb_topk_exact raised HDB_Q_UNDERFLOW and the packed manhattan flavour
returned scores of 0: profiles/low_score_contract_parent.log, figures in profiles/low_score_contract.txt."""
import numpy as np
import pytest

import lowscore

pytestmark = pytest.mark.gpu

N, K, TOL = lowscore.N_ROWS, lowscore.TOP_K, 1e-5


@pytest.fixture(scope="module")
def orc():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from oracle import ranking_oracle
    return ranking_oracle


def _host(t):
    return t.cpu().numpy()


def _worst(idx, sc, exact):
    """Largest score error of a batch's results in bands, and the number of queries that hold a row outside the band."""
    worst, bad = 0.0, 0
    for qi in range(idx.shape[0]):
        ref = exact[idx[qi], qi]
        r = np.abs(sc[qi].astype(np.float64) - ref) / lowscore.band_of(ref)
        worst = max(worst, float(r.max())); bad += bool(r.max() > 1.0)
    return worst, bad


# ------------------------------------------------------------------------------------------------
# B. low-score rows
# ------------------------------------------------------------------------------------------------
DOT_CASES = [(d, nq, K) for d, nq in lowscore.CASES] + [(384, 16, 2048)]


@pytest.mark.parametrize("d,nq,k", DOT_CASES)
def test_dot_product_holds_the_band_on_low_score_rows(orc, d, nq, k):
    """dot_product through the default call, the multi-kernel pipeline (use_batch1 = 0), with f32_split = 0 and on the VALU scan
    (use_mfma = 0): every query of every pass is a valid top k within 1e-5, the passes agree, no status word is raised.  The
    default call runs on the float32 matrix cores (mfma = 1, f32_split = 0): nothing divides a dot product by the norms, so the
    2^-17 |v| |q| of the bf16 parts is an error of several bands here."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q = lowscore.case(d, nq)
    exact = lowscore.exact_dot(d, nq)
    mid = METRIC_IDS["dot_product"]
    ix = GpuIndex(V)
    try:
        passes = {}
        for name, opt in (("default", None), ("pipeline", "use_batch1"), ("f32", "f32_split"), ("valu", "use_mfma")):
            if opt: ix.set_option(opt, 0)
            i_, s_, st_ = ix.topk_device(Q, k, mid)
            passes[name] = (_host(i_), _host(s_), int(st_.abs().sum().item()), ix.stat("mfma"), ix.stat("f32_split"), ix.stat("fused"))
            if opt: ix.set_option(opt, 1)
        for name, (i_, s_, st, mfma, f32s, fused) in passes.items():
            w, bad = _worst(i_, s_, exact)
            print(f"d={d} nq={nq} k={k} {name}: mfma={mfma} f32_split={f32s} fused={fused} status={st} worst error {w:.3f} bands, {bad} of {nq} queries outside")
        for name, (i_, s_, st, mfma, f32s, fused) in passes.items():
            assert st == 0, name
            for qi in range(nq):
                orc.check_topk(i_[qi], s_[qi], V, Q[qi], "dot_product", k, tol=TOL, exact=exact[:, qi])
        di, ds = passes["default"][:2]
        for name in ("pipeline", "f32", "valu"):
            oi, os_ = passes[name][:2]
            for qi in range(nq):
                assert orc.same_result_modulo_ties(di[qi], ds[qi], oi[qi], os_[qi], TOL), (name, qi)
        # the paths under test ran
        assert passes["default"][3:5] == (1, 0) and passes["pipeline"][3:5] == (1, 0) and passes["f32"][3:5] == (1, 0)
        assert passes["pipeline"][5] == 0 and passes["valu"][3:5] == (0, 0)
    finally:
        ix.close()


def _holds_band(idx, sc, exact, k, tol):
    """The band of the contract for a metric whose scores are far below 1: k distinct rows in descending order, every score within
    tol * max(1, |s|) of the float64-exact score of its row, and no row left out whose exact score beats the weakest returned one
    by more than two bands (two rows closer than that may swap when each is one band off).  check_topk's own left-out rule is
    RELATIVE to |s_k| (2e-7 for a cosine of 0.01) and asks for more than 1e-5 scores can order."""
    assert idx.shape == (k,) and np.unique(idx).size == k and np.all(sc[1:] <= sc[:-1])
    ref = exact[idx]
    assert np.all(np.abs(sc.astype(np.float64) - ref) <= tol * np.maximum(1.0, np.abs(ref)))
    rest = np.ones(exact.shape[0], dtype=bool); rest[idx] = False
    assert exact[rest].max() <= ref.min() + 2.0 * tol * max(1.0, abs(ref.min()))


@pytest.mark.parametrize("d,nq", lowscore.CASES)
def test_normalised_metrics_keep_the_parts_flavour_and_the_band(orc, d, nq):
    """cosine, euclidean and pearson on the same inputs: these still multiply as bf16 parts (f32_split = 1) -- what follows the
    product divides by |v| |q| or adds |v|^2 + |q|^2, so the same error is a small share of a band -- and must hold it."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q = lowscore.case(d, nq)
    ix = GpuIndex(V)
    try:
        for metric in ("cosine_similarity", "euclidean_metric", "pearson_correlation"):
            i_, s_, st_ = ix.topk_device(Q, K, METRIC_IDS[metric])
            assert ix.stat("mfma") == 1 and ix.stat("f32_split") == 1 and int(st_.abs().sum().item()) == 0, metric
            i_, s_ = _host(i_), _host(s_)
            for qi in range(nq):
                _holds_band(i_[qi], s_[qi], orc.exact_scores(V, Q[qi], metric), K, TOL)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------
# C. infinity and overflow edges
# ------------------------------------------------------------------------------------------------
def _split_finite(idx, sc):
    f = np.isfinite(sc)
    return (idx[f], sc[f]), (idx[~f], sc[~f])


@pytest.mark.parametrize("nq", [6, 40])
@pytest.mark.parametrize("dtype,d", [(np.float16, 96), (np.float16, 100), (np.float32, 100)])
def test_infinite_row_elements_on_padded_widths(orc, dtype, d, nq):
    """Rows narrower than the geometry they ride (hdb_mfma_anyd.h) meet zero query fragments past their end; the chunk fetched
    there is chunk 0 of the row again, and inf x 0 is NaN.  One row holds +inf in its first element, one -inf in its last; every
    query is non-zero there, so np.dot gives +-inf and never NaN.  The answer is the VALU scan's and a valid top k, infinite scores
    included, with the +inf rows first.  (fp16 d = 100 is no multiple of 16 bytes and has no matrix-core flavour: the control.)"""
    from hyperdb._native import GpuIndex, METRIC_IDS
    rng = np.random.default_rng(d * 131 + nq)
    r_pos, r_neg = 4242, N - 2                                  # (the second one in the ragged last tile)
    V = rng.standard_normal((N, d)).astype(dtype)
    V[r_pos, 0] = np.inf; V[r_neg, d - 1] = -np.inf
    Q = rng.standard_normal((nq, d)).astype(np.float32)
    Q[:, 0] = np.abs(Q[:, 0]) + 0.1                             # row r_pos scores +inf for every query
    Q[:, d - 1] = (np.abs(Q[:, d - 1]) + 0.1) * np.where(np.arange(nq) % 2 == 0, 1.0, -1.0)      # row r_neg: -inf for even queries, +inf for odd ones
    mid = METRIC_IDS["dot_product"]
    ix = GpuIndex(V)
    try:
        gi, gs, gst = ix.topk_device(Q, K, mid)
        gi, gs = _host(gi), _host(gs)
        assert int(gst.abs().sum().item()) == 0
        ix.set_option("use_mfma", 0)
        vi, vs, _ = ix.topk_device(Q, K, mid)
        vi, vs = _host(vi), _host(vs)
        assert ix.stat("mfma") == 0
        tol = orc.tolerance_for(dtype, "dot_product")
        with np.errstate(invalid="ignore", over="ignore"):
            for qi in range(nq):
                want_inf = [r_pos] if qi % 2 == 0 else [r_pos, r_neg]
                assert sorted(gi[qi][:len(want_inf)]) == want_inf and np.all(gs[qi][:len(want_inf)] == np.inf), qi
                (gfi, gfs), (gni, gns) = _split_finite(gi[qi], gs[qi])
                (vfi, vfs), (vni, vns) = _split_finite(vi[qi], vs[qi])
                assert sorted(gni) == sorted(vni) and np.array_equal(gns, vns), qi
                assert orc.same_result_modulo_ties(gfi, gfs, vfi, vfs, tol), qi
                orc.check_topk(gi[qi], gs[qi], V, Q[qi], "dot_product", K, tol=tol)
    finally:
        ix.close()


@pytest.mark.parametrize("d,nq", [(768, 8), (384, 16)])
def test_exact_call_answers_infinite_query_elements(orc, d, nq):
    """hdb_topk_exact is the last resort (the re-run of a call that raised a status word): it writes status 0 and the reference's
    answer whatever the query holds.  One query holds +inf, one -inf; the bf16 parts of an infinite value cancel to NaN, so an
    exact call with such a query does not multiply that way, and the two queries come back bit for bit as with f32_split = 0."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q0 = lowscore.case(d, nq)
    Q = Q0.copy()
    Q[2, 5] = np.inf; Q[5, d - 1] = -np.inf
    mid = METRIC_IDS["dot_product"]
    ix = GpuIndex(V)
    try:
        ei, es, est = ix.topk_device(Q, K, mid, exact=True)
        ei, es, est = _host(ei), _host(es), _host(est)
        assert ix.stat("path") == 2
        ix.set_option("f32_split", 0)
        fi, fs, _ = ix.topk_device(Q, K, mid, exact=True)
        fi, fs = _host(fi), _host(fs)
        ix.set_option("f32_split", 1)
        print(f"d={d} nq={nq} exact call: status {est.tolist()}")
        assert not est.any(), est.tolist()
        with np.errstate(invalid="ignore", over="ignore"):
            for qi in range(nq):
                orc.check_topk(ei[qi], es[qi], V, Q[qi], "dot_product", K, tol=TOL)
        for qi in (2, 5):
            assert np.array_equal(ei[qi], fi[qi]) and np.array_equal(es[qi].view(np.uint32), fs[qi].view(np.uint32)), qi
        # cosine keeps the bf16 parts in an exact call -- the default call's bits -- while no query holds an infinity, and drops
        # them for the whole call when one does: status 0 either way, and then the bits of f32_split = 0
        cid = METRIC_IDS["cosine_similarity"]
        di, ds, dst = ix.topk_device(Q0, K, cid)
        assert ix.stat("f32_split") == 1 and not _host(dst).any()
        ci, cs, cst = ix.topk_device(Q0, K, cid, exact=True)
        assert ix.stat("f32_split") == 1 and ix.stat("path") == 2 and not _host(cst).any()
        assert np.array_equal(_host(ci), _host(di)) and np.array_equal(_host(cs).view(np.uint32), _host(ds).view(np.uint32))
        ci, cs, cst = ix.topk_device(Q, K, cid, exact=True)
        assert ix.stat("f32_split") == 0 and ix.stat("mfma") == 1 and not _host(cst).any(), _host(cst).tolist()
        ix.set_option("f32_split", 0)
        gi, gs, _ = ix.topk_device(Q, K, cid, exact=True)
        ix.set_option("f32_split", 1)
        assert np.array_equal(_host(ci), _host(gi)) and np.array_equal(_host(cs).view(np.uint32), _host(gs).view(np.uint32))
        finite_q = [qi for qi in range(nq) if qi not in (2, 5)]
        for qi in finite_q:
            _holds_band(_host(ci)[qi], _host(cs)[qi], orc.exact_scores(V, Q[qi], "cosine_similarity"), K, TOL)
    finally:
        ix.close()


@pytest.mark.parametrize("q0", [-40000.0, -30000.0])
@pytest.mark.parametrize("nq", [2, 16])
def test_manhattan_tile_kernel_beyond_fp16_range(orc, nq, q0):
    """The tile kernel takes differences in packed fp16 when every query element is an fp16 number (hdb_l1_tile.hip).  v = 40000
    against q = -40000 (or -30000: both are fp16 numbers within range, their difference is not) rounds to inf there, the sum to inf,
    the score to 0.  The tile kernel must return the rows of the VALU scan (use_l1_tile = 0) with finite, positive scores within a
    relative 1e-3 of the float64-exact ones (scores are about 1e-5: the absolute band says nothing)."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    d = 384
    rng = np.random.default_rng(77 + nq)
    # the other 383 columns: N(0, 1) scaled row by row, so sum |v - q| runs from ~80 150 to ~86 000 (7 %: ranks far more than 1e-3 apart)
    V = (rng.standard_normal((N, d)) * rng.uniform(0.5, 20.0, size=(N, 1))).astype(np.float16)
    V[:, 0] = 40000.0
    Q = rng.standard_normal((nq, d)).astype(np.float16).astype(np.float32)
    Q[:, 0] = q0
    assert np.array_equal(Q.astype(np.float16).astype(np.float32), Q) and np.all(np.isfinite(V.astype(np.float32)))
    mid = METRIC_IDS["manhattan_distance"]
    ix = GpuIndex(V)
    try:
        ti, ts, tst = ix.topk_device(Q, K, mid)
        ti, ts = _host(ti), _host(ts)
        assert int(tst.abs().sum().item()) == 0
        ix.set_option("use_l1_tile", 0)
        vi, vs, _ = ix.topk_device(Q, K, mid)
        vi, vs = _host(vi), _host(vs)
        print(f"nq={nq} q0={q0}: scores {ts.max():.3e} .. {ts.min():.3e}")
        for qi in range(nq):
            exact = orc.exact_scores(V, Q[qi], "manhattan_distance")
            spread = exact.max() / exact.min() - 1.0
            assert spread > 0.01, spread
            rel = np.abs(ts[qi].astype(np.float64) - exact[ti[qi]]) / exact[ti[qi]]
            assert np.all(np.isfinite(ts[qi])) and np.all(ts[qi] > 0.0), qi
            assert np.array_equal(ti[qi], vi[qi]), qi
            assert rel.max() <= 1e-3, qi
            top = np.argsort(-exact, kind="stable")[:K]
            assert exact[ti[qi]].min() >= exact[top[-1]] * (1.0 - 2e-3), qi      # ... and they are the best rows
    finally:
        ix.close()
