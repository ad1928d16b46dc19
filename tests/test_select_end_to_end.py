"""The adversarial score arrays of tests/select_model.py through the public calls.  A float32 index with d = 1 and the query [1.0]
under dot_product scores row r as V[r, 0], exactly (one product, no sum), so a chosen score array reaches hdb_topk,
hdb_topk_exact and hdb_topk_host unchanged; the queries [-1.0], [2.0] and [0.5] of the same batch scale it exactly (-1.0 reverses
the order: the tie-heavy top level becomes the bottom one).  Indices and float32 score bits must equal the model's plain sort;
the `path` statistic is asserted in every case, so a plan change cannot move a case off the code it is meant for."""
import numpy as np
import pytest

import select_model as sm

pytestmark = pytest.mark.gpu

QUERIES = (1.0, -1.0, 2.0, 0.5)
STATUS_WORDS = {0, sm.Q_UNDERFLOW, sm.Q_OVERFLOW, sm.Q_UNDERFLOW | sm.Q_OVERFLOW}      # (no NaN anywhere in these calls)


def _specs(n, k):
    """Families of normal finite floats (no denormals, no infinities in the matrix), and signed zeros."""
    kk = min(k, n)
    return [
        ("gaussian", {}, "shuf"),
        ("one_level", {"value": 1.0}, None),
        ("levels", {"sizes": (kk // 2,), "tie": 1, "place": "last"}, None),
        ("levels", {"sizes": (kk // 2, n // 2), "tie": 1, "place": "inter"}, None),
        ("straddle", {"npos": n // 2, "band": 0}, "asc"),
        ("straddle", {"npos": kk // 3, "band": 0}, "shuf"),
        ("straddle", {"npos": kk // 2 + 600, "band": 600}, "desc"),
        ("ulp_chain", {"centre": 1.0, "byte": 0}, "shuf"),
        ("ulp_chain", {"centre": -1.0, "byte": 1}, "shuf"),
        ("full_range", {}, "shuf"),
        ("int_levels", {"d": 40}, "shuf"),
    ]


def _matrix_column(spec, n, seed):
    """The family's scores as a matrix column.  The lowest level of the level families is moved to zero first; every second zero
    of the column is stored as -0.0: it must come back as +0.0 and tie with the 0.0 rows by row order."""
    s = sm.make_scores(spec, n, seed)
    v = s.copy()
    if spec[0] in ("one_level", "levels", "int_levels"):
        v[v == v.min()] = 0.0
        s = v.copy()
    z = np.flatnonzero(v == 0.0)[::2]
    v[z] = -0.0
    assert not np.signbit(s[s == 0]).any()
    return s, v


def _expect(s, qv, n, k):
    with np.errstate(over="ignore"):                 # (3e38 * 2 is +inf in float32, in the kernel as here)
        return sm.topk(sm.canon(s * np.float32(qv)), n, k)


def _check(tag, idx, sc, s, qv, n, k):
    wi, wb = _expect(s, qv, n, k)
    bits = np.ascontiguousarray(sc).view(np.uint32)
    bad = np.flatnonzero((np.asarray(idx) != wi) | (bits != wb))
    assert bad.size == 0, "%s: %d of %d slots differ, first at %d: got (%d, %#010x) want (%d, %#010x)" % (
        tag, bad.size, k, bad[0], idx[bad[0]], bits[bad[0]], wi[bad[0]], wb[bad[0]])


def _run_calls(ix, s, Q, n, k, want_path, want_path_exact, tag, pins=()):
    """hdb_topk (raw status: a documented word; the answer where it is 0), hdb_topk_host (the model's answer always: it re-runs a
    call that reported a status) and hdb_topk_exact."""
    import torch
    from hyperdb._native import METRIC_IDS
    dot = METRIC_IDS["dot_product"]
    idx, sc, st = ix.topk_device(Q, k, dot)
    torch.cuda.synchronize()
    assert ix.stat("path") == want_path, (tag, ix.stat("path"))
    assert all(ix.stat(name) == v for name, v in pins), (tag, [(name, ix.stat(name)) for name, _ in pins])
    idx, sc, st = idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()
    for qi in range(len(Q)):
        assert int(st[qi]) in STATUS_WORDS, (tag, qi, st[qi])
        if st[qi] == 0:
            _check("%s hdb_topk q=%g" % (tag, Q[qi, 0]), idx[qi], sc[qi], s, Q[qi, 0], n, k)
        else:
            assert want_path == 1, (tag, qi, st[qi])            # only a sampled threshold may miss
    hi, hs, hst = ix.topk_views(Q, k, dot)
    for qi in range(len(Q)):
        _check("%s hdb_topk_host q=%g" % (tag, Q[qi, 0]), hi[qi].copy(), hs[qi].copy(), s, Q[qi, 0], n, k)
    assert (hst == 0).all(), (tag, hst)
    idx, sc, st = ix.topk_device(Q, k, dot, exact=True)
    torch.cuda.synchronize()
    assert ix.stat("path") == want_path_exact, (tag, ix.stat("path"))
    assert all(ix.stat(name) == v for name, v in pins), (tag, [(name, ix.stat(name)) for name, _ in pins])
    idx, sc, st = idx.cpu().numpy(), sc.cpu().numpy(), st.cpu().numpy()
    for qi in range(len(Q)):
        _check("%s hdb_topk_exact q=%g" % (tag, Q[qi, 0]), idx[qi], sc[qi], s, Q[qi, 0], n, k)
    assert (st == 0).all(), (tag, st)


# n -> (k, path of hdb_topk, path of hdb_topk_exact): 0 the small path, 1 the sampled path, 2 the exact path
PLANS = {8192: ((100, 0, 0), (2048, 0, 0)), 8193: ((100, 1, 2), (2048, 2, 2)), 20011: ((100, 1, 2), (2048, 2, 2))}


@pytest.mark.parametrize("n", sorted(PLANS))
def test_score_arrays_through_the_public_calls(n):
    from hyperdb._native import GpuIndex
    Q = np.array(QUERIES, dtype=np.float32).reshape(4, 1)
    for k, path, path_exact in PLANS[n]:
        for i, spec in enumerate(_specs(n, k)):
            s, v = _matrix_column(spec, n, 300 + i)
            ix = GpuIndex(v.reshape(n, 1))
            try:
                _run_calls(ix, s, Q, n, k, path, path_exact, "n=%d k=%d %s" % (n, k, sm.spec_name(spec)))
            finally:
                ix.close()


@pytest.mark.parametrize("n", sorted(PLANS))
def test_sixteen_byte_rows_single_query(n):
    """d = 4, rows [v, 0, 0, 0], the query [1, 0, 0, 0], use_mfma at its default.  The plan reports, for every n and k here,
    mfma = 0 and fused = 0 with path 0 (n = 8192), 1 (sampled) or 2 (exact): a single float32 query rides the VALU scan, whose
    v * 1 + 0 * 0 + 0 * 0 + 0 * 0 is exact, so the case stays at the default use_mfma and no matrix-core flavour is involved."""
    from hyperdb._native import GpuIndex
    Q = np.array([[1.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    for k, path, path_exact in PLANS[n]:
        for i, spec in enumerate(_specs(n, k)[::2]):
            s, v = _matrix_column(spec, n, 500 + i)
            V = np.zeros((n, 4), dtype=np.float32)
            V[:, 0] = v
            ix = GpuIndex(V)
            try:
                tag = "d=4 n=%d k=%d %s" % (n, k, sm.spec_name(spec))
                _run_calls(ix, s, Q, n, k, path, path_exact, tag, pins=(("mfma", 0), ("fused", 0)))
            finally:
                ix.close()
