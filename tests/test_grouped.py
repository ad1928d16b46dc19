"""Grouped top-k on the GPU: the best row per group, k distinct groups per query (hdb_topk_grouped_host, hdb_collapse_groups).

Integer data (|x| <= 8, d = 64, dot product) are scored exactly by every arithmetic the library has, so those answers are compared for
equality with a numpy int64 model of the contract: order the eligible rows by (score descending, row ascending), keep each group's
first row, take the first k.  Float data are held to the project's bands (1e-5 * max(1, |s|), 1e-3 for float16) against float64
scores, where the band only decides ties.  Every path of the call is pinned by construction through its statistics."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D_INT = 64
NQ_INT = (1, 4, 5, 9)
K_INT = (1, 10, 100)
_cache = {}


# ------------------------------------------------------------------------------------------------ the model
def model_grouped(scores, groups, k, eligible=None):
    """scores: [nq, n] (int64 or float64) -> (rows [nq, k] int64, -1 padded).  The contract, in numpy."""
    nq, n = scores.shape
    rows = np.arange(n)
    out = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        order = np.lexsort((rows, -scores[q]))
        if eligible is not None:
            order = order[eligible[order]]
        _, first = np.unique(groups[order], return_index=True)
        first.sort()
        reps = order[first[:k]]
        out[q, :len(reps)] = reps
    return out


def _int_data(n):
    """Integer rows and queries, the float64 score matrix of all nine queries and the four group layouts: built once per n."""
    if ("int", n) not in _cache:
        rng = np.random.default_rng(n)
        V = rng.integers(-8, 9, size=(n, D_INT)).astype(np.int64)
        Q = rng.integers(-8, 9, size=(max(NQ_INT), D_INT)).astype(np.int64)
        S = Q @ V.T
        runs = np.repeat(np.arange(n), rng.integers(1, 9, size=n))[:n]                    # contiguous runs of 1 .. 8 rows
        runs = np.unique(runs, return_inverse=True)[1].reshape(-1)
        layouts = {"runs": runs, "shuffled": rng.permutation(runs), "one": np.zeros(n, np.int64), "each": np.arange(n)}
        expect = {(name, k): model_grouped(S, g, k) for name, g in layouts.items() for k in K_INT}
        for a in (V, Q, S, *layouts.values(), *expect.values()):
            a.setflags(write=False)
        _cache[("int", n)] = (V, Q, S, layouts, expect)
    return _cache[("int", n)]


def _make_index(V, storage):
    from hyperdb._native import GpuIndex
    if storage == "float32":
        return GpuIndex(V.astype(np.float32))
    if storage == "float16":
        return GpuIndex(V.astype(np.float16))
    if storage == "bfloat16":
        return GpuIndex(torch.from_numpy(V.astype(np.float32)).to(torch.bfloat16).cuda())
    if storage == "float8":
        return GpuIndex(torch.from_numpy(V.astype(np.float32)).to(torch.float8_e4m3fn).cuda())
    return GpuIndex(V.astype(np.int8), storage="int8")


def _status(ix, nq, k):
    return ix._host_records[(nq, k)][4].copy()


# ------------------------------------------------------------------------------------------------ exact equality on integer data
@pytest.mark.parametrize("n", [3_000, 20_001])
@pytest.mark.parametrize("storage", ["float32", "float16", "bfloat16", "int8", "float8"])
def test_integer_data_equal_the_model(storage, n):
    """Indices, scores and group ids equal the int64 model on every storage, both sizes (the small path and one above 8192 rows with
    an odd tail), nq = 1, 4, 5, 9, k = 1, 10, 100 and the four group layouts -- through the default schedule and, with
    group_fast_rounds = 0, through the exact grouped pass alone."""
    from hyperdb._native import METRIC_IDS
    V, Q, S, layouts, expect = _int_data(n)
    ix = _make_index(V, storage)
    try:
        mid = METRIC_IDS["dot_product"]
        Qf = Q.astype(np.float32)
        for name, g in layouts.items():
            ix.set_groups(g)
            assert ix.n_groups == int(g.max()) + 1
            for rounds in (2, 0):
                ix.set_option("group_fast_rounds", rounds)
                for nq in NQ_INT:
                    for k in K_INT:
                        idx, sc = ix.topk_grouped(Qf[:nq], k, mid)
                        want = expect[(name, k)][:nq]
                        where = (storage, n, name, rounds, nq, k)
                        assert ix.stat("grouped") == 1, where
                        if rounds == 0:
                            assert ix.stat("group_rounds") == 0 and ix.stat("group_exact") == nq, where
                        assert np.array_equal(idx, want), (where, idx[0][:12], want[0][:12])
                        live = want >= 0
                        want_s = np.where(live, np.take_along_axis(S[:nq], np.maximum(want, 0), axis=1), 0).astype(np.float64)
                        assert np.array_equal(np.where(live, sc.astype(np.float64), 0.0), want_s), where
                        assert np.isneginf(sc[~live]).all(), where
                        gi = g[np.maximum(idx, 0)]
                        for q in range(nq):                                            # no group twice
                            assert len(set(gi[q][live[q]].tolist())) == int(live[q].sum()), where
                        assert (_status(ix, nq, k) == 0).all(), where
            ix.set_option("group_fast_rounds", 2)
        # an ungrouped call afterwards is an ungrouped call
        ix.topk(Qf[:1], 5, mid)
        assert ix.stat("grouped") == 0 and ix.stat("group_rounds") == 0
    finally:
        ix.close()


def test_bits_index_equals_the_model():
    """A packed-bit index (storage="bits"): 0/1 rows against small-integer queries are exact as well."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q, S, layouts, expect = _int_data(20_001)
    bits = V > 0
    Sb = Q @ bits.astype(np.int64).T
    ix = GpuIndex(np.packbits(bits, axis=1), storage="bits")
    try:
        for name in ("runs", "shuffled"):
            g = layouts[name]
            ix.set_groups(g)
            for rounds in (2, 0):
                ix.set_option("group_fast_rounds", rounds)
                for nq, k in ((1, 10), (5, 100)):
                    idx, sc = ix.topk_grouped(Q[:nq].astype(np.float32), k, METRIC_IDS["dot_product"])
                    want = model_grouped(Sb[:nq], g, k)
                    assert np.array_equal(idx, want), (name, rounds, nq, k)
                    assert np.array_equal(sc.astype(np.int64), np.take_along_axis(Sb[:nq], want, axis=1)), (name, rounds, nq, k)
    finally:
        ix.close()


def test_rank_grouped_returns_group_ids():
    import hyperdb.ranking_algorithm as ranking
    V, Q, S, layouts, expect = _int_data(3_000)
    g = layouts["shuffled"]
    idx, sc, gid = ranking.rank_grouped(V.astype(np.float32), Q[:4].astype(np.float32), g, top_k=10, metric="dot_product")
    want = expect[("shuffled", 10)][:4]
    assert idx.dtype == np.int64 and sc.dtype == np.float64 and gid.dtype == np.int64
    assert np.array_equal(idx, want) and np.array_equal(gid, g[want])
    assert np.array_equal(sc, np.take_along_axis(S[:4], want, axis=1).astype(np.float64))
    # one group: one hit and the -1 / -inf / -1 tail
    idx, sc, gid = ranking.rank_grouped(V.astype(np.float32), Q[:2].astype(np.float32), layouts["one"], top_k=3, metric="dot_product")
    assert np.array_equal(idx[:, 0], expect[("one", 1)][:2, 0]) and (idx[:, 1:] == -1).all() and (gid[:, 1:] == -1).all() and np.isneginf(sc[:, 1:]).all()


# ------------------------------------------------------------------------------------------------ each path pinned by construction
def _stepped(n_groups_rows, d=16):
    """Rows whose column 0 holds a per-group value, strictly decreasing over the groups; the query e0 then scores a group's rows
    alike.  n_groups_rows: rows per group, in order."""
    sizes = np.asarray(n_groups_rows)
    groups = np.repeat(np.arange(len(sizes)), sizes)
    V = np.zeros((len(groups), d), np.float32)
    V[:, 0] = (len(sizes) - groups).astype(np.float32)
    return V, groups


def test_second_round_is_pinned():
    """Contiguous groups of 12 rows, k = 10, oversample 4: the top 40 rows hold 4 groups, the top 160 hold 14."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, groups = _stepped([12] * 250)
    Q = np.zeros((3, 16), np.float32)
    Q[:, 0] = (1.0, 2.0, 3.0)
    ix = GpuIndex(V)
    try:
        ix.set_groups(groups)
        idx, sc = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert (ix.stat("group_rounds"), ix.stat("group_k"), ix.stat("group_exact")) == (2, 160, 0)
        want = np.tile(np.arange(10) * 12, (3, 1))
        assert np.array_equal(idx, want)
        assert np.array_equal(sc, Q[:, :1] * (250 - np.arange(10, dtype=np.float32))[None, :])
        ix.set_option("group_fast_rounds", 1)                    # one round only: the short queries go to the exact pass
        idx1, sc1 = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert (ix.stat("group_rounds"), ix.stat("group_k"), ix.stat("group_exact")) == (1, 40, 3)
        ix.set_option("group_fast_rounds", 0)
        idx0, sc0 = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert (ix.stat("group_rounds"), ix.stat("group_k"), ix.stat("group_exact")) == (0, 0, 3)
        for a, b in ((idx1, sc1), (idx0, sc0)):
            assert np.array_equal(a, idx) and np.array_equal(b, sc)
        ix.set_option("group_fast_rounds", 2)
        ix.set_option("group_oversample", 16)                    # 160 rows at once: one round
        idx16, sc16 = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert (ix.stat("group_rounds"), ix.stat("group_k"), ix.stat("group_exact")) == (1, 160, 0)
        assert np.array_equal(idx16, idx) and np.array_equal(sc16, sc)
    finally:
        ix.close()


@pytest.mark.parametrize("small_groups", [500, 4_000])
def test_one_huge_group_takes_the_exact_pass(small_groups):
    """One group of 3 000 top rows before many small groups: no fast round can see a second group.  4 000 small groups of two rows
    put the matrix above 8192 rows."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, groups = _stepped([3_000] + [2] * small_groups)
    Q = np.zeros((3, 16), np.float32)
    Q[:, 0] = (1.0, 2.0, 3.0)
    ix = GpuIndex(V)
    try:
        ix.set_groups(groups)
        idx, sc = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert ix.stat("group_exact") == 3 and ix.stat("grouped") == 1
        if small_groups == 500:                                  # (the small path never fails: both rounds ran, and both were short)
            assert (ix.stat("group_rounds"), ix.stat("group_k")) == (2, 160)
        want = np.concatenate([[0], 3_000 + 2 * np.arange(9)])
        assert np.array_equal(idx, np.tile(want, (3, 1)))
        assert np.array_equal(sc, Q[:, :1] * (small_groups + 1 - np.arange(10, dtype=np.float32))[None, :])
        ix.set_option("group_fast_rounds", 0)
        idx0, sc0 = ix.topk_grouped(Q, 10, METRIC_IDS["dot_product"])
        assert ix.stat("group_exact") == 3 and np.array_equal(idx0, idx) and np.array_equal(sc0, sc)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ float data against the oracle
N_F, D_F, NQ_F, K_F = 20_001, 96, 5, 10
FOUR = ("cosine_similarity", "euclidean_metric", "manhattan_distance", "pearson_correlation")


def _float_data(dt):
    if ("float", dt) not in _cache:
        rng = np.random.default_rng(7 if dt == np.float32 else 8)
        V = rng.standard_normal((N_F, D_F)).astype(np.float32).astype(dt)
        Q = rng.standard_normal((NQ_F, D_F)).astype(np.float32).astype(dt).astype(np.float32)     # queries that the stored type holds
        groups = np.unique(np.repeat(np.arange(N_F), rng.integers(1, 9, size=N_F))[:N_F], return_inverse=True)[1].reshape(-1)
        mask = rng.random(N_F) < 1.0 / 3.0
        bias = (rng.random(N_F) * 0.1).astype(np.float32)
        for a in (V, Q, groups, mask, bias):
            a.setflags(write=False)
        _cache[("float", dt)] = (V, Q, groups, mask, bias)
    return _cache[("float", dt)]


def _ref_scores(dt, metric, filtered):
    from oracle import ranking_oracle as orc
    key = ("ref", dt, metric, filtered)
    if key not in _cache:
        V, Q, groups, mask, bias = _float_data(dt)
        S = np.stack([orc.exact_scores(V, Q[q], metric, bias=bias if filtered else None) for q in range(NQ_F)])
        if filtered:
            S[:, ~mask] = -np.inf
        best = np.full((NQ_F, int(groups.max()) + 1), -np.inf)
        for q in range(NQ_F):
            np.maximum.at(best[q], groups, S[q])
        S.setflags(write=False)
        best.setflags(write=False)
        _cache[key] = (S, best)
    return _cache[key]


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("metric", FOUR)
@pytest.mark.parametrize("dt", [np.float32, np.float16])
def test_float_data_against_the_oracle(dt, metric, filtered):
    """Gaussian rows: no group twice, every returned row is in its group and within the band of its group's best, scores descend,
    every group not returned has its best at most the k-th returned score plus the band.  Default schedule and exact pass."""
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q, groups, mask, bias = _float_data(dt)
    S, best = _ref_scores(dt, metric, filtered)
    band = 1e-3 if dt == np.float16 else 1e-5
    ix = GpuIndex(V)
    try:
        ix.set_groups(groups)
        if filtered:
            ix.set_row_mask(mask.astype(np.uint8))
            ix.set_bias(bias)
        for rounds in (2, 0):
            ix.set_option("group_fast_rounds", rounds)
            idx, sc = ix.topk_grouped(Q, K_F, METRIC_IDS[metric])
            for q in range(NQ_F):
                where = (dt.__name__, metric, filtered, rounds, q)
                rows, got = idx[q], sc[q].astype(np.float64)
                assert (rows >= 0).all() and np.isfinite(got).all(), where
                g = groups[rows]
                assert len(set(g.tolist())) == K_F, where                                  # no group twice
                if filtered:
                    assert mask[rows].all(), where
                tol = band * np.maximum(1.0, np.abs(S[q][rows]))
                assert (np.abs(got - S[q][rows]) <= tol).all(), (where, np.abs(got - S[q][rows]).max())
                assert (S[q][rows] >= best[q][g] - tol).all(), where                       # its group's best, or tied with it
                assert (got[:-1] >= got[1:]).all(), where                                  # scores descend
                others = np.ones(best.shape[1], bool)
                others[g] = False
                kth = got[-1]
                assert best[q][others].max() <= kth + band * max(1.0, abs(kth)), (where, best[q][others].max(), kth)
    finally:
        ix.close()


def test_fast_path_equals_the_collapsed_ungrouped_call():
    """With no query in the exact pass the answer IS collapse_groups_host(topk(Q, group_k)) of the same handle, bit for bit."""
    from hyperdb._native import GpuIndex, METRIC_IDS, collapse_groups_host
    for dt in (np.float32, np.float16):
        V, Q, groups, mask, bias = _float_data(dt)
        ix = GpuIndex(V)
        try:
            ix.set_groups(groups)
            for nq in (1, 4, 5):
                idx, sc = ix.topk_grouped(Q[:nq], K_F, METRIC_IDS["cosine_similarity"])
                assert ix.stat("group_exact") == 0 and ix.stat("group_rounds") == 1
                kr = ix.stat("group_k")
                assert kr == 4 * K_F
                li, ls = ix.topk(Q[:nq], kr, METRIC_IDS["cosine_similarity"])
                wi, ws, wst = collapse_groups_host(li, ls, groups, K_F)
                assert np.array_equal(idx, wi) and np.array_equal(sc.view(np.uint32), ws.view(np.uint32)) and (wst == 0).all(), (dt.__name__, nq)
        finally:
            ix.close()


# ------------------------------------------------------------------------------------------------ the primitive alone
@pytest.mark.parametrize("m", [1, 63, 64, 65, 2048])
def test_collapse_primitive_against_its_model(m):
    from hyperdb import _native
    rng = np.random.default_rng(m)
    n, G = 5_000, 700
    groups = rng.integers(0, G, size=n)
    nq = 4
    idx = np.stack([rng.permutation(n)[:m] for _ in range(nq)]).astype(np.int64)
    sc = -np.sort(-rng.standard_normal((nq, m)).astype(np.float32), axis=1)
    if m > 1:
        idx[1, m // 2:], sc[1, m // 2:] = -1, -np.inf                  # a -1 tail: exhaustive
        idx[2] = np.flatnonzero(groups == groups[idx[2, 0]])[0]        # one group (one row, listed m times)
        idx[3, m // 3] = n + 17                                        # an id outside the index
    for k in sorted({1, min(m, 10), m}):
        gi, gs, gst = _native.collapse_groups(idx, sc, groups, k)
        wi, ws, wst = _native.collapse_groups_host(idx, sc, groups, k)
        gi, gs, gst = gi.cpu().numpy(), gs.cpu().numpy(), gst.cpu().numpy()
        assert np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32)), (m, k)
        assert np.array_equal(gst, wst), (m, k, gst, wst)
        if m > 1:
            assert gst[1] == 0                                         # short, but exhaustive
            assert gst[3] & _native.Q_BADROW and not gst[0] & _native.Q_BADROW
            if k > 1:
                assert gst[2] == _native.Q_GROUPS_SHORT and (gi[2, 1:] == -1).all()
            # the bad id changes nothing else: the answer is that of the list without the entry
            keep = np.arange(m) != m // 3
            ci, cs, _ = _native.collapse_groups_host(idx[3:4, keep], sc[3:4, keep], groups, min(k, m - 1))
            assert np.array_equal(gi[3, :min(k, m - 1)], ci[0]) and np.array_equal(gs[3, :min(k, m - 1)], cs[0])
    # the whole ranking (m = n) is never short
    if m == 64:
        small = groups[:64] % 3
        li = rng.permutation(64)[None, :].astype(np.int64)
        ls = -np.sort(-rng.standard_normal((1, 64)).astype(np.float32), axis=1)
        gi, gs, gst = _native.collapse_groups(li, ls, small, 10)
        assert gst.cpu().numpy().tolist() == [0] and (gi.cpu().numpy()[0, 3:] == -1).all()


def test_collapse_composes_with_a_row_base_and_device_lists():
    """The output of topk_device goes in as it is (CUDA tensors, row_base added)."""
    from hyperdb import _native
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q, S, layouts, expect = _int_data(3_000)
    base = 1_000_000
    ix = GpuIndex(V.astype(np.float32), row_base=base)
    try:
        li, ls, lst = ix.topk_device(Q[:4].astype(np.float32), 200, METRIC_IDS["dot_product"])
        g = layouts["runs"]
        gi, gs, gst = _native.collapse_groups(li, ls, g, 10, row_base=base)
        assert np.array_equal(gi.cpu().numpy() - base, expect[("runs", 10)][:4]) and (gst.cpu().numpy() == 0).all()
        # without the base every id is outside the index: skipped and flagged, nothing read
        gi, gs, gst = _native.collapse_groups(li, ls, g, 10)
        assert (gi.cpu().numpy() == -1).all() and (gst.cpu().numpy() & _native.Q_BADROW).all()
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ bad group ids in a device tensor
@pytest.mark.parametrize("n", [3_000, 20_001])
def test_bad_group_ids_count_as_masked(n):
    """Through the C entry (the Python check would refuse them): rows whose id is outside [0, n_groups) behave as masked rows,
    HDB_Q_BADROW is set, no other row's answer changes.  The ids are compared, never used."""
    from hyperdb import _native
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q, S, layouts, expect = _int_data(n)
    g = layouts["runs"].astype(np.int64)
    n_groups = int(g.max()) + 1
    rng = np.random.default_rng(n + 1)
    bad_rows = rng.choice(n, size=n // 10, replace=False)
    bad_rows = np.union1d(bad_rows, model_grouped(S[:1], g, 3)[0])            # the very best rows among them
    gb = g.copy()
    gb[bad_rows] = rng.choice(np.array([-5, -1, n_groups, n_groups + 3, 2 ** 31 - 1, -2 ** 31]), size=len(bad_rows))
    ok = np.ones(n, bool)
    ok[bad_rows] = False
    dev = torch.from_numpy(gb.astype(np.int32)).cuda()
    ix = GpuIndex(V.astype(np.float32))
    lib = _native.lib()
    try:
        mid = METRIC_IDS["dot_product"]
        Qf = Q[:4].astype(np.float32)
        for k in (10, 100):
            want = model_grouped(S[:4], g, k, eligible=ok)
            for rounds in (2, 0):
                ix.set_option("group_fast_rounds", rounds)
                assert lib.hdb_index_set_groups(ix._h, ctypes.c_void_p(dev.data_ptr()), n_groups) == 0
                idx, sc = ix.topk_grouped(Qf, k, mid)
                st = _status(ix, 4, k)
                assert np.array_equal(idx, want), (n, k, rounds)
                assert np.array_equal(sc.astype(np.int64), np.take_along_axis(S[:4], want, axis=1)), (n, k, rounds)
                if rounds == 0:
                    assert (st == _native.Q_BADROW).all(), (n, k, rounds, st)
                else:
                    assert (st & ~_native.Q_BADROW == 0).all() and st[0] == _native.Q_BADROW, (n, k, rounds, st)
        # the primitive with the same ids
        li, ls, _ = ix.topk_device(Qf, 400, mid)
        gi, gs, gst = _native.collapse_groups(li, ls, dev, 10, n_groups=n_groups)
        assert np.array_equal(gi.cpu().numpy(), model_grouped(S[:4], g, 10, eligible=ok))
        assert (gst.cpu().numpy() & _native.Q_BADROW)[0]
    finally:
        assert lib.hdb_index_set_groups(ix._h, None, 0) == 0
        ix.close()


# ------------------------------------------------------------------------------------------------ lifecycle
def test_groups_follow_the_matrix_lifecycle():
    from hyperdb import _native
    from hyperdb._native import GpuIndex, METRIC_IDS
    V, Q, S, layouts, expect = _int_data(3_000)
    Vf, Qf, mid = V.astype(np.float32), Q[:2].astype(np.float32), METRIC_IDS["dot_product"]
    g = layouts["runs"]
    ix = GpuIndex(Vf[:2_000])
    try:
        with pytest.raises(ValueError, match="no groups set"):
            ix.topk_grouped(Qf, 5, mid)
        ix.set_groups(g[:2_000])
        first = ix.topk_grouped(Qf, 5, mid)[0]
        assert np.array_equal(first, model_grouped(S[:2, :2_000], g[:2_000], 5))
        # rebase keeps the ids
        assert _native.lib().hdb_index_rebase(ix._h, ctypes.c_void_p(ix.V.data_ptr())) == 0
        assert np.array_equal(ix.topk_grouped(Qf, 5, mid)[0], first)
        # append, update and compact drop them with mask and bias
        ix.append(Vf[2_000:])
        with pytest.raises(ValueError, match="no groups set"):
            ix.topk_grouped(Qf, 5, mid)
        with pytest.raises(ValueError, match="one entry per row"):
            ix.set_groups(g[:2_000])
        ix.set_groups(g)
        assert np.array_equal(ix.topk_grouped(Qf, 5, mid)[0], expect[("runs", 10)][:2, :5])
        ix.update(Vf)
        with pytest.raises(ValueError, match="no groups set"):
            ix.topk_grouped(Qf, 5, mid)
        ix.set_groups(g)
        assert np.array_equal(ix.topk_grouped(Qf, 5, mid)[0], expect[("runs", 10)][:2, :5])
        keep = np.flatnonzero(np.arange(3_000) % 3 != 1)
        ix.compact(keep)
        with pytest.raises(ValueError, match="no groups set"):
            ix.topk_grouped(Qf, 5, mid)
        ix.set_groups(g[keep])
        assert np.array_equal(keep[ix.topk_grouped(Qf, 5, mid)[0]], keep[model_grouped(S[:2][:, keep], g[keep], 5)])
        ix.set_groups(None)
        with pytest.raises(ValueError, match="no groups set"):
            ix.topk_grouped(Qf, 5, mid)
        # what is not built says so
        ix.set_groups(g[keep])
        with pytest.raises(NotImplementedError):
            ix.topk_grouped(Qf, 5, METRIC_IDS["hamming_distance"])
        with pytest.raises(NotImplementedError):
            ix.topk_grouped(Qf, 2049, mid)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------ facade
def _collapse_results(res, key, k):
    """The host model over the facade's own ungrouped answer: the first result of each group, k of them."""
    seen, out = set(), []
    for doc, score, src in res:
        gk = key(doc, src)
        if gk in seen:
            continue
        seen.add(gk)
        out.append((doc, score, src))
    return out[:k]


def _same(got, want, sources=True):
    assert [d["name"] for d, _, _ in got] == [d["name"] for d, _, _ in want]
    if sources:
        assert [s for _, _, s in got] == [s for _, _, s in want]
    for (_, a, _), (_, b, _) in zip(got, want):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(b))


def test_facade_group_by():
    from hyperdb import HyperDB
    rng = np.random.default_rng(5)
    n, d = 600, 32
    V = rng.standard_normal((n, d)).astype(np.float32)
    docs = [{"name": f"doc{i}", "info": {"type": f"t{i % 7}"} if i % 5 else {}} for i in range(n)]
    db = HyperDB(documents=docs, vectors=V, metadata_keys=["info.type"])
    db.source_indices = [i // 4 for i in range(n)]                    # a loaded store of chunked documents: four chunks each
    q = rng.standard_normal(d).astype(np.float32)
    by_source = lambda doc, src: src
    by_type = lambda doc, src: doc["info"].get("type", doc["name"])
    plain = db.query(q, top_k=8)
    full = db.query(q, top_k=n)
    _same(db.query_grouped(q, "source", top_k=8), _collapse_results(full, by_source, 8))
    _same(db.query_grouped(q, "info.type", top_k=20), _collapse_results(full, by_type, 20))
    # more groups asked for than exist: the shorter list
    kept = [("metadata", {"info.type": "t3"})]
    got = db.query_grouped(q, "info.type", top_k=5, filters=kept)
    assert len(got) == 1 and got[0][0]["info"]["type"] == "t3"
    _same(got, _collapse_results(db.query(q, top_k=n, filters=kept), by_type, 5))
    # a metadata key with a filter
    odd = [("mask", np.arange(n) % 2 == 1)]
    _same(db.query_grouped(q, "source", top_k=12, filters=odd, metric="euclidean_metric"),
          _collapse_results(db.query(q, top_k=n, filters=odd, metric="euclidean_metric"), by_source, 12))
    # a batch
    Qb = rng.standard_normal((3, d)).astype(np.float32)
    for qi, res in enumerate(db.query_batch(Qb, top_k=6, group_by="source")):
        _same(res, _collapse_results(db.query(Qb[qi], top_k=n), by_source, 6))
    # after a removal: tombstoned device rows.  (remove_document renumbers source_indices by VALUE, as the reference does for its
    # one-vector-per-document stores; a chunked store states the sources of the documents it kept.)
    db.remove_document([0, 1, 2, 3, 17, 250])
    db.source_indices = [int(doc["name"][3:]) // 4 for doc in db.documents]
    assert db._dead.size == 6
    full = db.query(q, top_k=len(db.documents))
    _same(db.query_grouped(q, "source", top_k=8), _collapse_results(full, by_source, 8))
    _same(db.query_grouped(q, "info.type", top_k=9), _collapse_results(full, by_type, 9))
    # group_by = None is the ungrouped call, and the ungrouped call is what it was
    # (a fresh store of the same documents, every document its own source: documents and scores are those of the first call)
    db2 = HyperDB(documents=[dict(x) for x in docs], vectors=V, metadata_keys=["info.type"])
    again = db2.query(q, top_k=8)
    _same(again, plain, sources=False)
    _same(db2.query_grouped(q, None, top_k=8), again)
    _same(db2.query_batch(q.reshape(1, -1), top_k=8, group_by=None)[0], again)
    _same(db2.query_grouped(q, "source", top_k=8), again)              # one document per source: grouping changes nothing
    with pytest.raises(ValueError, match="group_by"):
        db2.query_grouped(q, "colour")
