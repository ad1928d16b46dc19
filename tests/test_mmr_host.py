"""Host side of the diverse top-k (hdb_mmr, hdb_mmr_host): the ABI, the argument errors that are decided before any HIP call, the
Python signatures, the numpy model of the contract on hand-written lists, the refusal of handles that are not one index on one
device, and the plan and workspace of the call (csrc/hdb_mmr_plan.h, MmrWs).  No GPU is used."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hdb_mmr", "hdb_mmr_host")
NINF = -np.inf


def _err(lib):
    return lib.hdb_last_error().decode()


def test_version_exports_and_prototypes():
    from hyperdb import _native
    assert _native.lib().hdb_version() >= 112
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    header = open(os.path.join(ROOT, "include", "hyperdb_hip.h")).read()
    assert "int hdb_mmr(hdb_index* ix, const int64_t* dev_idx, const float* dev_score, int32_t nq, int32_t m, int32_t k, double lambda," in header
    assert "int hdb_mmr_host(hdb_index* ix, const void* dev_Q, int32_t nq, int32_t m, int32_t k, int metric, double lambda, int pair_metric," in header
    for word in ("mmr_chunks", "one-workgroup flavour", "on the fly", "matrix cores for the pair pass", "m > 2048", "several GPUs / shards",
                 "val of each pick"):
        assert word in header, word


def test_python_signatures_and_defaults():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb import HyperDB, _native
    from hyperdb._native import GpuIndex
    s = inspect.signature(GpuIndex.mmr_device).parameters
    assert list(s)[:6] == ["self", "idx", "scores", "k", "lambda_mult", "pair_metric_id"]
    assert s["lambda_mult"].default == 0.5 and s["pair_metric_id"].default is None
    s = inspect.signature(GpuIndex.mmr).parameters
    assert list(s) == ["self", "Q", "m", "k", "metric_id", "lambda_mult", "pair_metric_id"]
    assert s["lambda_mult"].default == 0.5 and s["pair_metric_id"].default is None
    s = inspect.signature(_native.mmr_host).parameters
    assert list(s) == ["V", "idx", "scores", "k", "lambda_mult", "pair_metric", "row_base"] and s["row_base"].default == 0
    s = inspect.signature(ranking.rank_mmr).parameters
    assert list(s) == ["vectors", "query_vectors", "top_k", "fetch_k", "lambda_mult", "metric", "pair_metric", "timestamps", "recency_bias"]
    assert s["top_k"].default == 5 and s["fetch_k"].default is None and s["lambda_mult"].default == 0.5
    assert s["metric"].default == "cosine_similarity" and s["pair_metric"].default is None
    assert s["timestamps"].default is None and s["recency_bias"].default == 0
    assert "rank_mmr" in ranking.__all__
    s = inspect.signature(HyperDB.query_diverse).parameters
    assert list(s) == ["self", "query_input", "top_k", "fetch_k", "lambda_mult", "return_similarities", "filters", "recency_bias", "timestamp_key",
                       "metric"]
    assert s["top_k"].default == 5 and s["fetch_k"].default is None and s["lambda_mult"].default == 0.5 and s["return_similarities"].default is True
    assert s["filters"].default is None and s["recency_bias"].default == 0 and s["timestamp_key"].default is None
    assert s["metric"].default == "cosine_similarity"
    # HyperDB.query keeps the reference's parameter list
    assert list(inspect.signature(HyperDB.query).parameters) == ["self", "query_input", "top_k", "return_similarities", "filters", "recency_bias",
                                                                 "timestamp_key", "metric", "ann_percent"]


def test_sharded_handles_are_refused():
    """A handle that is not one index on one device is refused before anything else is looked at."""
    import hyperdb.ranking_algorithm as ranking
    sharded = ranking.ResidentVectors.__new__(ranking.ResidentVectors)
    sharded.index = object()
    with pytest.raises(NotImplementedError, match="one device"):
        ranking.rank_mmr(sharded, "not even an array")
    from hyperdb.group import GpuGroup
    with pytest.raises(NotImplementedError, match="one device"):
        ranking.rank_mmr(GpuGroup.__new__(GpuGroup), np.zeros((1, 4)))


def test_argument_errors_before_any_hip_call():
    """Sizes, lambda and the pair metric are judged first, from the numbers alone; then the handle.  A NULL handle is never
    dereferenced and the list pointers are never read."""
    from hyperdb import _native
    lib = _native.lib()
    p = ctypes.c_void_p(64)          # a non-null pointer that is never read: every call below fails before it would be
    mmr = lambda nq, m, k, lam=0.5, pm=1, ix=None: lib.hdb_mmr(ix, p, p, nq, m, k, lam, pm, p, p, p, None)
    host = lambda nq, m, k, lam=0.5, pm=1, metric=1, ix=None: lib.hdb_mmr_host(ix, p, nq, m, k, metric, lam, pm, p, None)
    for call, who in ((mmr, "hdb_mmr:"), (host, "hdb_mmr_host:")):
        for m in (0, 2049, -3):
            assert call(2, m, 1) == -1 and "[1, 2048]" in _err(lib) and who in _err(lib), (who, m, _err(lib))
        for m, k in ((10, 0), (10, 11), (1, 2), (2048, 2049), (10, -1)):
            assert call(2, m, k) == -1 and "[1, m]" in _err(lib) and who in _err(lib), (who, m, k, _err(lib))
        for lam in (-0.1, 1.5, float("nan"), float("inf")):
            assert call(2, 10, 5, lam=lam) == -1 and "lambda" in _err(lib) and who in _err(lib), (who, lam, _err(lib))
        for pm in (3, 4, 5, 6, 7, -1, 99):
            assert call(2, 10, 5, pm=pm) == -3 and "pair_metric" in _err(lib) and who in _err(lib), (who, pm, _err(lib))
        assert call(-1, 10, 5) == -1 and "nq" in _err(lib) and who in _err(lib)
        # the largest list, k = m and both ends of lambda pass the size checks: the NULL handle fails
        for lam in (0.0, 1.0):
            assert call(2, 2048, 2048, lam=lam) == -1 and "null" in _err(lib) and who in _err(lib)
        for pm in (0, 1, 2):
            assert call(2, 1, 1, pm=pm) == -1 and "null" in _err(lib)
    # no query: nothing to do, once the sizes have passed ...
    assert mmr(0, 0, 1) == -1 and "[1, 2048]" in _err(lib)
    assert mmr(0, 10, 5) == 0
    # ... and the one-call form takes no empty batch
    assert host(0, 10, 5) == -1 and "positive" in _err(lib)
    with pytest.raises(NotImplementedError):
        _native._check(mmr(1, 10, 5, pm=4), "hdb_mmr")
    with pytest.raises(ValueError):
        _native._check(mmr(1, 10, 5, lam=2.0), "hdb_mmr")


# ---- the numpy model on hand-written lists -------------------------------------------------------------------------------------
def _rows():
    """Six rows in the plane: 0 and 1 are copies, 2 is close to them, 3 and 4 point elsewhere, 5 is the zero row."""
    return np.array([[1.0, 0.0], [1.0, 0.0], [0.9, 0.1], [0.0, 1.0], [-1.0, 0.0], [0.0, 0.0]])


def test_model_padding_neg_inf_repeat_and_bad_ids():
    from hyperdb._native import mmr_host, Q_BADROW
    V = _rows()
    idx = np.array([[100, -1, 102, 100, 103, 999, 104, 50]], dtype=np.int64)
    sc = np.array([[0.9, 0.95, 0.8, 0.99, NINF, 0.7, 0.1, 0.6]], dtype=np.float32)
    # candidates in list order: 100 (0.9), 102 (0.8), 104 (0.1); -1 is padding, the second 100 a repeat (its 0.99 is never seen), 103 sits
    # at -inf, 999 and 50 lie outside [100, 106)
    i, s, st = mmr_host(V, idx, sc, 4, 1.0, "dot_product", row_base=100)
    assert i.tolist() == [[100, 102, 104, -1]] and st.tolist() == [Q_BADROW]
    assert s[0, :3].tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.1)] and s[0, 3] == NINF
    # without the two outside ids the status is clean
    i2, _, st2 = mmr_host(V, idx[:, :5], sc[:, :5], 2, 1.0, "dot_product", row_base=100)
    assert i2.tolist() == [[100, 102]] and st2.tolist() == [0]
    # row_base = 0: 100 .. 104 are outside, 50 too; nothing is left
    i3, s3, st3 = mmr_host(V, idx, sc, 2, 0.5, "cosine_similarity")
    assert i3.tolist() == [[-1, -1]] and np.all(s3 == NINF) and st3.tolist() == [Q_BADROW]


def test_model_all_padding_and_fewer_candidates_than_k():
    from hyperdb._native import mmr_host
    V = _rows()
    i, s, st = mmr_host(V, np.full((2, 3), -1), np.zeros((2, 3), np.float32), 3, 0.5, "cosine_similarity")
    assert i.tolist() == [[-1] * 3] * 2 and np.all(s == NINF) and st.tolist() == [0, 0]
    i, s, st = mmr_host(V, np.array([[3, -1, 4, -1]]), np.array([[0.5, 0.9, 0.7, 0.8]], np.float32), 4, 0.5, "cosine_similarity")
    assert i.tolist() == [[4, 3, -1, -1]] and s[0, :2].tolist() == [np.float32(0.7), np.float32(0.5)] and np.all(s[0, 2:] == NINF)


def test_model_lambda_one_is_the_ranking_and_lambda_zero_flees_the_picks():
    from hyperdb._native import mmr_host
    V = _rows()
    idx = np.array([[2, 0, 3, 1, 4]], dtype=np.int64)
    sc = np.array([[0.8, 0.9, 0.3, 0.9, 0.2]], dtype=np.float32)
    # lambda = 1: relevance descending, position ascending -- the tie of rows 0 and 1 goes to row 0, which stands first
    for pm in ("dot_product", "cosine_similarity", "euclidean_metric"):
        i, s, _ = mmr_host(V, idx, sc, 5, 1.0, pm)
        assert i.tolist() == [[0, 1, 2, 3, 4]], pm
        assert s.tolist() == [[np.float32(x) for x in (0.9, 0.9, 0.8, 0.3, 0.2)]]
    # lambda = 0: relevance decides step 0 alone (row 0, the first of the tie); then the row least like any pick: the opposite row 4
    # (cosine -1), then row 3 (0 to both), then row 2 (0.99 to row 0) and last the copy, row 1 (cosine 1)
    i, s, _ = mmr_host(V, idx, sc, 5, 0.0, "cosine_similarity")
    assert i.tolist() == [[0, 4, 3, 2, 1]]
    assert s.tolist() == [[np.float32(x) for x in (0.9, 0.2, 0.3, 0.8, 0.9)]]          # the relevances, in pick order
    # in between: 0.5 * r - 0.5 * pen -- after row 0, the copy (0.45 - 0.5) loses to row 3 (0.15 - 0) and row 4 (0.1 + 0.5)
    i, _, _ = mmr_host(V, idx, sc, 3, 0.5, "cosine_similarity")
    assert i.tolist() == [[0, 4, 3]]


def test_model_ties_go_to_the_lowest_position_at_every_step():
    from hyperdb._native import mmr_host
    # rows 0 .. 3 orthogonal unit vectors, equal relevance: every step is a tie of all that is left
    V = np.eye(4)
    i, _, _ = mmr_host(V, np.array([[2, 0, 3, 1]]), np.full((1, 4), 0.5, np.float32), 4, 0.5, "dot_product")
    assert i.tolist() == [[2, 0, 3, 1]]
    # a candidate whose value is -inf is still picked when nothing better is left: the dot product of rows 0 and 1 overflows float32,
    # so after row 0 the penalty of row 1 is +inf and its value -inf; row 2 goes first, then row 1
    big = np.array([[2.0e19, 0.0], [2.0e19, 0.0], [0.0, 1.0]])
    i, s, _ = mmr_host(big, np.array([[0, 1, 2]]), np.array([[1.0, 0.9, -1.0]], np.float32), 3, 0.25, "dot_product")
    assert i.tolist() == [[0, 2, 1]] and s[0].tolist() == [np.float32(1.0), np.float32(-1.0), np.float32(0.9)]
    V = _rows()
    # pair metric by id, and one that is no pair metric
    i2, _, _ = mmr_host(V, np.array([[0, 5]]), np.array([[1.0, 0.5]], np.float32), 2, 0.25, 0)
    assert i2.tolist() == [[0, 5]]
    with pytest.raises(NotImplementedError):
        mmr_host(V, np.array([[0, 5]]), np.array([[1.0, 0.5]], np.float32), 2, 0.25, "manhattan_distance")


def test_model_val_is_float32_with_every_step_rounded():
    """lam * r and oml * pen are rounded to float32 before the subtraction: two candidates that a float64 evaluation separates tie in
    float32, and the lower position wins."""
    from hyperdb._native import mmr_host
    V = np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]])
    r = np.float32(1.0)
    r_up = np.nextafter(r, np.float32(2.0), dtype=np.float32)
    # after row 0 (relevance 2): candidates 1 and 2 have pen 0; 0.1f * 1.0f and 0.1f * nextafter(1.0f) differ in float64 and round
    # to the same float32 or to neighbours -- the model must do what float32 arithmetic does, whatever that is
    sc = np.array([[2.0, r, r_up]], np.float32)
    i, _, _ = mmr_host(V, np.array([[0, 1, 2]]), sc, 3, 0.1, "dot_product")
    lam = np.float32(0.1)
    want = [0, 1, 2] if lam * r >= lam * r_up else [0, 2, 1]
    assert i.tolist() == [want]


def test_mmr_plan_and_workspace(tmp_path):
    """tests/mmr_plan_check.hip, compiled and run like tests/group_plan_check.hip: host code under AddressSanitizer and UBSan.  cq over
    (nq, m, exact_bytes), tile and grid counts, size equals placement."""
    host_check.run(host_check.build("mmr_plan_check", tmp_path))
