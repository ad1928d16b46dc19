"""hdb_rerank: the exact top-k of every query among ITS OWN list of rows, and the two-stage call built on it.

The contract (include/hyperdb_hip.h): a returned row carries the float32 bits the VALU scan gives that row on this handle, i.e. the
indices and score bits of topk_device(exact=True) with use_mfma = use_fused = use_quant = use_l1_tile = 0 (and auto_quant = 0) under
a row mask that keeps exactly the query's valid candidates; padding (-1), ids outside the index, masked rows and repeats drop out;
status is 0, Q_NAN or Q_BADROW.

Base matrix: 20 001 Gaussian rows (not a multiple of 16), one seeded matrix per (dtype, d), shared and never changed.  Lists: random
order, row 0 and row n - 1 in every list, a tenth of the slots -1 in random places, one row listed three times, different per query.
The ABI wants k <= m, so the calls take k = min(10, m): m = 5 (three distinct rows) and k = m = 1000 exercise the -1 / -inf tail.
The masked exact call lists masked rows at -inf where fewer than k rows are kept; the comparison reads such an entry as the
-1 / -inf padding the rerank contract prescribes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 20_001
K = 10
M_ALL = (1, 5, 16, 17, 1000, 8192)
NQS = (1, 3, 9)
FIVE = ("dot_product", "cosine_similarity", "euclidean_metric", "manhattan_distance", "pearson_correlation")
THREE = ("dot_product", "euclidean_metric", "manhattan_distance")
_TORCH = {"f16": torch.float16, "f32": torch.float32, "f64": torch.float64, "bf16": torch.bfloat16}
_CACHE = {}


def _matrix(dt, d, n=N):
    """(what GpuIndex takes, storage keyword) of the seeded matrix."""
    key = ("V", dt, d, n)
    if key not in _CACHE:
        from hyperdb import _native
        g = np.random.default_rng(4000 + d).standard_normal((n, d))
        if dt == "i8":
            _CACHE[key] = (np.clip(np.rint(g * 40), -127, 127).astype(np.int8), "int8")
        elif dt == "f8":
            _CACHE[key] = (_native.to_f8(g.astype(np.float32)), None)
        else:
            _CACHE[key] = (torch.from_numpy(g).to(_TORCH[dt]).contiguous(), None)
    return _CACHE[key]


def _index(dt, d, n=N, row_base=0, valu=True):
    from hyperdb._native import GpuIndex
    v, storage = _matrix(dt, d, n)
    ix = GpuIndex(v, row_base=row_base, storage=storage)
    if valu:
        for name in ("use_mfma", "use_fused", "use_quant", "use_l1_tile", "auto_quant"):
            ix.set_option(name, 0)
    return ix


def _queries(dt, d, nq, seed=5):
    return np.random.default_rng(seed + d).standard_normal((nq, d)).astype(np.float64 if dt == "f64" else np.float32)


def _bias(n=N):
    return np.random.default_rng(3).uniform(-0.5, 0.5, n).astype(np.float32)


def _lists(m, nq, seed=0, n=N):
    """[nq, m] int64: see the module docstring.  m = 1 alternates between row 0 and row n - 1."""
    key = ("L", m, nq, seed, n)
    if key not in _CACHE:
        rng = np.random.default_rng(900 + 31 * m + 7 * nq + seed)
        out = np.empty((nq, m), np.int64)
        for q in range(nq):
            if m == 1:
                out[q, 0] = 0 if q % 2 == 0 else n - 1
                continue
            pad, dup = m // 10, 2 if m >= 5 else 0
            inner = rng.choice(np.arange(1, n - 1), size=m - pad - dup - 2, replace=False)
            ids = np.concatenate([[0, n - 1], inner])
            row = np.concatenate([ids, np.full(dup, ids[-1]), np.full(pad, -1)]).astype(np.int64)
            out[q] = rng.permutation(row)
        _CACHE[key] = out
    return _CACHE[key]


def _valid(row, n=N, base=0, keep=None):
    ids = np.unique(row[(row >= base) & (row < base + n)]) - base
    return ids if keep is None else ids[keep[ids] != 0]


def _np(t3):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in t3)


def _rerank(ix, Q, cand, k, metric):
    from hyperdb._native import METRIC_IDS
    return _np(ix.rerank_device(Q, cand, k, METRIC_IDS[metric]))


def _reference(ix, Q, cand, k, metric, handle_mask=None):
    """Per query: the masked exact VALU call of the same handle, its -inf entries of rows the mask drops read as padding."""
    from hyperdb._native import METRIC_IDS
    n, base = ix.n, ix.row_base
    idx, sc, st = [], [], []
    try:
        for q in range(Q.shape[0]):
            ids = _valid(cand[q], n, base, handle_mask)
            mk = np.zeros(n, np.uint8)
            mk[ids] = 1
            ix.set_row_mask(mk)
            i, s, t = _np(ix.topk_device(Q[q:q + 1], k, METRIC_IDS[metric], exact=True))
            drop = np.isneginf(s[0]) & ~np.isin(i[0] - base, ids)
            idx.append(np.where(drop, -1, i[0])); sc.append(s[0]); st.append(t[0])
    finally:
        ix.set_row_mask(handle_mask)
    return np.stack(idx), np.stack(sc), np.array(st)


def _same_bits(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and np.array_equal(a[2], b[2])


def _ulps(a, b):
    ka, kb = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ka, kb = np.where(ka < 0, -(ka & 0x7FFFFFFF), ka), np.where(kb < 0, -(kb & 0x7FFFFFFF), kb)
    return int(np.abs(ka - kb).max()) if ka.size else 0


def _sweep(dt, d, metric, biases):
    ix = _index(dt, d)
    calls, misses = 0, []                    # every call is compared; the figures are printed before the assertion
    try:
        for with_bias in biases:
            ix.set_bias(_bias() if with_bias else None)
            for m in M_ALL:
                for nq in NQS:
                    ix.set_option("rerank_chunk", 4 if nq == 9 else 0)
                    Q, cand = _queries(dt, d, nq), _lists(m, nq)
                    for k in ((min(K, m), m) if m == 1000 and nq == 3 else (min(K, m),)):
                        got = _rerank(ix, Q, cand, k, metric)
                        assert ix.stat("rerank") == 1 and ix.stat("chunks") == (3 if nq == 9 else 1)
                        want = _reference(ix, Q, cand, k, metric)
                        assert ix.stat("rerank") == 0 and ix.stat("mfma") == 0 and ix.stat("fused") == 0 and ix.stat("quant") == 0
                        calls += 1
                        if not _same_bits(got, want):
                            misses.append((m, nq, k, with_bias, "idx" if not np.array_equal(got[0], want[0]) else "",
                                           "status" if not np.array_equal(got[2], want[2]) else "", f"{_ulps(got[1], want[1])} ulp"))
                        for q in range(nq):
                            nv = len(_valid(cand[q]))
                            assert (got[0][q, :min(nv, k)] >= 0).all() and (got[0][q, nv:] == -1).all() and np.isneginf(got[1][q, nv:]).all()
                            assert np.isin(got[0][q][got[0][q] >= 0], cand[q]).all()
                        assert (got[2] == 0).all()
    finally:
        ix.close()
    print(f"{dt} d={d} {metric}: {len(misses)} of {calls} calls differ from the masked exact VALU call")
    for miss in misses[:20]:
        print("   ", miss)
    assert not misses, (dt, d, metric, len(misses), calls, misses[:5])


# fp16 x 384: unrolled 768-byte rows; float32 x 96: 384 bytes, a ragged second step
@pytest.mark.parametrize("metric", FIVE)
@pytest.mark.parametrize("dt,d", [("f16", 384), ("f32", 96)])
def test_bits_of_the_valu_scan_full_cross(dt, d, metric):
    _sweep(dt, d, metric, (False, True))


# float32 x 100: 25 pieces, the runtime loop with a ragged step; fp16 x 300: 600 bytes, the element loop; float64; bf16;
# float8 / int8 x 384: 24 pieces of sixteen one-byte elements; int8 x 130: the element loop
@pytest.mark.parametrize("metric", THREE)
@pytest.mark.parametrize("dt,d", [("f32", 100), ("f16", 300), ("f64", 64), ("bf16", 128), ("f8", 384), ("i8", 384), ("i8", 130)])
def test_bits_of_the_valu_scan_other_shapes(dt, d, metric):
    _sweep(dt, d, metric, (True,))


@pytest.mark.parametrize("metric", FIVE)
@pytest.mark.parametrize("dt,d", [("f16", 384), ("f32", 96), ("f64", 64), ("bf16", 128), ("f8", 384), ("i8", 384)])
def test_reference_arithmetic(dt, d, metric):
    """oracle.check_topk on V[ids] with bias[ids] at the dtype's tolerance, indices mapped back."""
    from oracle import ranking_oracle as orc
    ix = _index(dt, d, valu=False)
    try:
        Vh, bias = ix.host_matrix(), _bias()
        ix.set_bias(bias)
        Q, cand = _queries(dt, d, 3), _lists(1000, 3)
        idx, sc, st = _rerank(ix, Q, cand, K, metric)
        assert (st == 0).all()
        for q in range(3):
            ids = _valid(cand[q])
            pos = np.searchsorted(ids, idx[q])
            assert np.array_equal(ids[pos], idx[q])
            orc.check_topk(pos, sc[q], Vh[ids], Q[q], metric, K, bias=bias[ids], tol=orc.tolerance_for(np.float16 if dt == "f16" else np.float32, metric))
    finally:
        ix.close()


@pytest.mark.parametrize("dt,d,metric", [("f16", 384, "cosine_similarity"), ("f32", 100, "euclidean_metric"), ("i8", 130, "manhattan_distance")])
def test_position_independence(dt, d, metric):
    """The same lists shuffled, and the same candidates padded into a longer m, return identical bits."""
    ix = _index(dt, d)
    try:
        ix.set_bias(_bias())
        rng = np.random.default_rng(8)
        Q, cand = _queries(dt, d, 3), _lists(1000, 3)
        a = _rerank(ix, Q, cand, K, metric)
        shuffled = np.stack([rng.permutation(r) for r in cand])
        padded = np.full((3, 1500), -1, np.int64)
        for q in range(3):
            padded[q, rng.choice(1500, 1000, replace=False)] = cand[q]
        alone = [_rerank(ix, Q[q:q + 1], cand[q:q + 1], K, metric) for q in range(3)]      # ... nor on the other queries
        for b in (_rerank(ix, Q, shuffled, K, metric), _rerank(ix, Q, padded, K, metric), tuple(np.concatenate(x) for x in zip(*alone))):
            assert _same_bits(a, b)
    finally:
        ix.close()


def test_mask_row_base_and_row_list():
    dt, d, metric, base = "f32", 96, "cosine_similarity", 1_000_000
    Q, cand = _queries(dt, d, 3), _lists(1000, 3)
    ix, ixb = _index(dt, d), _index(dt, d, row_base=base)
    try:
        for h in (ix, ixb):
            h.set_bias(_bias())
        plain = _rerank(ix, Q, cand, K, metric)
        # a handle mask that drops a third of the rows: they never appear, and the rest score as before
        mask = (np.arange(N) % 3 != 1).astype(np.uint8)
        ix.set_row_mask(mask)
        got = _rerank(ix, Q, cand, K, metric)
        assert (mask[got[0]] == 1).all() and (got[0] >= 0).all() and not _same_bits(got, plain)
        assert _same_bits(got, _reference(ix, Q, cand, K, metric, handle_mask=mask))
        # a row list set on the handle changes nothing
        rows = np.flatnonzero(mask).astype(np.int64)
        ix.set_row_subset(mask, rows)
        assert ix.stat("subset_rows") == len(rows)
        assert _same_bits(got, _rerank(ix, Q, cand, K, metric))
        ix.set_row_mask(None)
        # an index with a base takes and returns based ids
        based = np.where(cand >= 0, cand + base, cand)
        gb = _rerank(ixb, Q, based, K, metric)
        assert _same_bits((gb[0] - base, gb[1], gb[2]), plain)
        assert _same_bits(gb, _reference(ixb, Q, based, K, metric))
    finally:
        ix.close()
        ixb.close()


def test_validation():
    from hyperdb._native import GpuIndex, METRIC_IDS, Q_BADROW, Q_NAN
    dt, d, metric, base = "f32", 96, "dot_product", 1_000_000
    Q = _queries(dt, d, 3)
    for rb in (0, base):
        ix = _index(dt, d, row_base=rb)
        try:
            cand = _lists(1000, 3).copy()
            cand[cand >= 0] += rb
            clean, dirty = cand.copy(), cand.copy()
            slots = [3, 500, 999] if rb else [3, 500]
            bad = [N + rb, 2 ** 40, rb - 1][:len(slots)]
            clean[1, slots], dirty[1, slots] = -1, bad
            want = _rerank(ix, Q, clean, K, metric)
            dev = torch.from_numpy(dirty).to(ix.device)
            got = _rerank(ix, Q, dev, K, metric)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
            assert got[2].tolist() == [0, Q_BADROW, 0] and (want[2] == 0).all()
            with pytest.raises(IndexError):
                ix.rerank(Q, dev, K, METRIC_IDS[metric])
            with pytest.raises(IndexError):
                ix.rerank(Q, dirty, K, METRIC_IDS[metric])             # a host array: refused before any GPU call
            gi, gs = ix.rerank(Q, clean, K, METRIC_IDS[metric])
            assert np.array_equal(gi, want[0]) and np.array_equal(gs.view(np.uint32), want[1].view(np.uint32))
            # a NaN query
            Qn = Q.copy()
            Qn[2, 5] = np.nan
            st = _rerank(ix, Qn, clean, K, metric)[2]
            assert st.tolist() == [0, 0, Q_NAN]
            with pytest.raises(ValueError):
                ix.rerank(Qn, clean, K, METRIC_IDS[metric])
            for m_ in ("hamming_distance", "jaccard_similarity"):
                with pytest.raises(NotImplementedError):
                    ix.rerank_device(Q, clean, K, METRIC_IDS[m_])
            with pytest.raises(ValueError):
                ix.rerank_device(Q, clean[:, :5], K, METRIC_IDS[metric])        # k > m
        finally:
            ix.close()
    bits = GpuIndex(np.random.default_rng(1).standard_normal((500, 96)) > 0, storage="bits")
    try:
        with pytest.raises(NotImplementedError):
            bits.rerank_device(Q, np.zeros((3, 4), np.int64), 2, METRIC_IDS["dot_product"])
    finally:
        bits.close()


def _two_stage_pair(second_dt, n=N, d=384, first_rows=None):
    """first = storage="bits" over V > 0 (or over `first_rows`), second = int8 or fp16 over V."""
    from hyperdb._native import GpuIndex
    v, storage = _matrix(second_dt, d, n)
    vh = v if isinstance(v, np.ndarray) else v.float().numpy()
    first = GpuIndex((vh > 0) if first_rows is None else first_rows, storage="bits")
    second = GpuIndex(v, storage=storage)
    return first, second, vh


def _composed(first, second, Q, Q1, top_k, k1, metric, first_metric):
    import hyperdb.ranking_algorithm as ranking
    c = ranking.rank_batch(first, Q1, top_k=k1, metric=first_metric)[0]
    return ranking.rerank_batch(second, Q, c, top_k=top_k, metric=metric)


def _same_ranked(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].astype(np.float32).view(np.uint32), b[1].astype(np.float32).view(np.uint32))


@pytest.mark.parametrize("second_dt", ["i8", "f16"])
def test_two_stage_is_the_composition_of_its_stages(second_dt):
    import hyperdb.ranking_algorithm as ranking
    first, second, _ = _two_stage_pair(second_dt)
    try:
        Q = _queries("f32", 384, 9)
        Qp = np.packbits(Q > 0, axis=1)
        for fm, Q1 in (("cosine_similarity", Q), ("hamming_distance", Qp)):
            got = ranking.rank_two_stage(first, second, Q, top_k=K, oversample=4, metric="cosine_similarity", first_metric=fm,
                                         first_queries=None if Q1 is Q else Q1)
            assert second.stat("rerank") == 1 and got[0].shape == (9, K) and got[0].dtype == np.int64 and got[1].dtype == np.float64
            want = _composed(first, second, Q, Q1, K, 4 * K, "cosine_similarity", fm)
            assert _same_ranked(got, want), fm
            assert (got[0] >= 0).all() and (np.diff(got[1], axis=1) <= 0).all()
        # defaults: first_metric = metric, first_queries = query_vectors
        assert _same_ranked(ranking.rank_two_stage(first, second, Q, top_k=K), _composed(first, second, Q, Q, K, 4 * K, "cosine_similarity", "cosine_similarity"))
    finally:
        first.close()
        second.close()


def test_two_stage_with_every_row_a_candidate_is_the_exact_top_k():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb._native import METRIC_IDS
    n = 8000
    first, second, _ = _two_stage_pair("i8", n=n)
    try:
        Q = _queries("f32", 384, 3)
        got = ranking.rank_two_stage(first, second, Q, top_k=K, oversample=1000, metric="cosine_similarity")      # k1 = min(10 000, 8192, n) = n
        for name in ("use_mfma", "use_fused", "use_quant", "use_l1_tile"):
            second.set_option(name, 0)
        wi, ws, wst = _np(second.topk_device(Q, K, METRIC_IDS["cosine_similarity"], exact=True))
        assert (wst == 0).all() and _same_ranked(got, (wi, ws))
    finally:
        first.close()
        second.close()


def test_two_stage_survives_a_failing_first_stage():
    """40 distinct first-stage rows repeated to 20 001: every score is a 500-fold tie.  With the sampled threshold aimed at 16
    survivors (sample_target, as tests/test_row_subset.py fails a sampled pass) the threshold sits on the best level, its 500 rows
    pass and k1 = 600 are wanted: the first stage reports that in its status words (asserted, so the input is what it claims).
    The call re-runs those queries exactly and returns the composed answer; afterwards `first` reports the statistics of its first
    attempt, all of them, not those of the last one-query exact re-run."""
    import hyperdb.ranking_algorithm as ranking
    from hyperdb._native import METRIC_IDS
    rng = np.random.default_rng(12)
    rows = (rng.standard_normal((40, 384)) > 0)[np.arange(N) % 40]
    first, second, _ = _two_stage_pair("i8", first_rows=rows)
    try:
        first.set_option("sample_target", 16)
        Q = _queries("f32", 384, 3)
        k1 = 60 * K
        st = _np(first.topk_device(Q, k1, METRIC_IDS["cosine_similarity"]))[2]
        print("first-stage status words:", st.tolist())
        assert (st != 0).any()
        attempt = {s: first.stat(s) for s in ("path", "mfma", "fused", "chunks", "quant")}
        got = ranking.rank_two_stage(first, second, Q, top_k=K, oversample=60, metric="cosine_similarity")
        print("first-stage statistics:", attempt)
        assert {s: first.stat(s) for s in attempt} == attempt
        assert _same_ranked(got, _composed(first, second, Q, Q, K, k1, "cosine_similarity", "cosine_similarity"))
        assert (got[0] >= 0).all()
    finally:
        first.close()
        second.close()


def test_two_stage_refuses_mismatched_handles():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb._native import GpuIndex
    first, second, vh = _two_stage_pair("i8", n=8000)
    shorter = GpuIndex(vh[:7000] > 0, storage="bits")
    based = GpuIndex(vh > 0, storage="bits", row_base=5)
    group = ranking.register_vectors(vh.astype(np.float32), devices=[0, 0])
    try:
        Q = _queries("f32", 384, 2)
        for bad in (shorter, based):
            with pytest.raises(ValueError):
                ranking.rank_two_stage(bad, second, Q)
        with pytest.raises(NotImplementedError):
            ranking.rank_two_stage(first, group, Q)
        with pytest.raises(NotImplementedError):
            ranking.rerank_batch(group, Q, np.zeros((2, 4), np.int64))
    finally:
        for h in (first, second, shorter, based, group):
            h.close()


def test_nothing_else_moved():
    """A plain top-k on the same handle returns what it returned before the rerank calls, and its stats are its own."""
    from hyperdb._native import METRIC_IDS
    dt, d = "f16", 384
    ix = _index(dt, d, valu=False)
    try:
        Q = _queries(dt, d, 9)
        before = {m_: _np(ix.topk_device(Q, K, METRIC_IDS[m_])) for m_ in ("cosine_similarity", "euclidean_metric")}
        stats = {s: ix.stat(s) for s in ("path", "mfma", "fused", "chunks")}
        ix.set_option("rerank_chunk", 4)
        for m_ in FIVE:
            _rerank(ix, Q, _lists(1000, 9), K, m_)
            assert ix.stat("rerank") == 1 and ix.stat("chunks") == 3 and ix.stat("mfma") == 0 and ix.stat("path") == 0
        for m_, want in before.items():
            assert _same_bits(_np(ix.topk_device(Q, K, METRIC_IDS[m_])), want)
            assert ix.stat("rerank") == 0
        assert {s: ix.stat(s) for s in stats} == stats
    finally:
        ix.close()
