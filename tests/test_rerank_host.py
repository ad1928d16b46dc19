"""Host side of hdb_rerank / hdb_rerank_host / hdb_two_stage_host: the ABI, the argument errors that are decided before any HIP call,
the candidate check of the Python binding and the workspace layout (RerankWs, csrc/hdb_ws.h).  No GPU is used."""
import ctypes
import os

import numpy as np
import pytest
import torch

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hdb_rerank", "hdb_rerank_host", "hdb_two_stage_host")


def test_version_and_exports():
    from hyperdb import _native
    assert _native.lib().hdb_version() >= 109
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.Q_BADROW == 8 and _native.CAND_CAP == 8192
    header = open(os.path.join(ROOT, "include", "hyperdb_hip.h")).read()
    assert "HDB_Q_BADROW = 8" in header


def _err(lib):
    return lib.hdb_last_error().decode()


def test_argument_errors_before_any_hip_call():
    """Sizes are judged first, from the numbers alone; then the handle.  A NULL handle is never dereferenced."""
    from hyperdb import _native
    lib = _native.lib()
    p = ctypes.c_void_p(64)          # a non-null pointer that is never read: every call below fails before it would be
    calls = {
        "hdb_rerank": lambda ix, nq, m, k: lib.hdb_rerank(ix, p, nq, p, m, k, 1, p, p, p, None),
        "hdb_rerank_host": lambda ix, nq, m, k: lib.hdb_rerank_host(ix, p, nq, p, m, k, 1, p, None),
        "hdb_two_stage_host": lambda ix, nq, m, k: lib.hdb_two_stage_host(ix, p, 1, m, ix, p, 1, k, nq, p, None),
    }
    for name, call in calls.items():
        assert call(None, 2, 100, 10) == -1 and "null" in _err(lib) and name in _err(lib), (name, _err(lib))
        for m, k, word in ((0, 1, "[1, 8192]"), (8193, 10, "[1, 8192]"), (-5, 1, "[1, 8192]"), (100, 101, "[1, m]"), (100, 0, "[1, m]"), (1, 2, "[1, m]")):
            assert call(None, 2, m, k) == -1, (name, m, k)
            assert word in _err(lib) and name in _err(lib), (name, m, k, _err(lib))
        assert call(None, -1, 100, 10) == -1 and "nq" in _err(lib), name
    # the largest list and k = m pass the size check: what fails is the handle
    assert calls["hdb_rerank"](None, 1, 8192, 8192) == -1 and "null index" in _err(lib)
    # the host entries need at least one query; hdb_rerank takes none and does nothing
    assert calls["hdb_rerank_host"](None, 0, 100, 10) == -1 and "positive" in _err(lib)
    assert calls["hdb_two_stage_host"](None, 0, 100, 10) == -1 and "positive" in _err(lib)


def test_check_candidates():
    from hyperdb._native import check_candidates
    n, base = 1000, 0
    good = np.array([[0, 5, 999, -1], [7, 7, -1, -1]])
    assert check_candidates(good, 2, n, base) == 4
    for dt in (np.int32, np.int64, np.uint32, np.int16):
        assert check_candidates(np.array([[0, 5, 999]], dtype=dt), 1, n, base) == 3
    assert check_candidates(torch.tensor([[0, 999, -1]], dtype=torch.int64), 1, n, base) == 3
    assert check_candidates([[1, 2], [3, 4]], 2, n, base) == 2
    assert check_candidates(np.full((1, 8192), -1), 1, n, base) == 8192
    for bad in (np.array([1, 2, 3]), np.zeros((2, 3, 4), np.int64), np.zeros((2, 0), np.int64), np.zeros((1, 8193), np.int64),
                np.array([[0.5, 2.0]]), np.array([[True, False]]), torch.tensor([[0.5]]), np.zeros((3, 4), np.int64)):
        with pytest.raises(ValueError):
            check_candidates(bad, 2, n, base)
    with pytest.raises(IndexError, match="1000"):
        check_candidates(np.array([[0, 1000], [1, 2]]), 2, n, base)
    with pytest.raises(IndexError, match=str(2 ** 40)):
        check_candidates(np.array([[0, 2 ** 40]]), 1, n, base)
    # with a base: ids are global; n + row_base is the first id past the end, row_base - 1 the last one before it; -1 stays padding
    base = 1_000_000
    assert check_candidates(np.array([[base, base + n - 1, -1, -7]]), 1, n, base) == 4
    with pytest.raises(IndexError, match=str(base + n)):
        check_candidates(np.array([[base, base + n]]), 1, n, base)
    with pytest.raises(IndexError, match=str(base - 1)):
        check_candidates(torch.tensor([[base - 1, base]]), 1, n, base)
    with pytest.raises(IndexError, match="5"):
        check_candidates(np.array([[5]]), 1, n, base)


def test_python_entry_points_exist():
    import inspect
    import hyperdb.ranking_algorithm as ranking
    from hyperdb._native import GpuIndex
    assert list(inspect.signature(ranking.rerank_batch).parameters) == ["vectors", "query_vectors", "candidates", "top_k", "metric", "timestamps", "recency_bias"]
    assert list(inspect.signature(ranking.rank_two_stage).parameters) == ["first", "second", "query_vectors", "top_k", "oversample", "metric", "first_metric", "first_queries"]
    sig = inspect.signature(ranking.rank_two_stage).parameters
    assert sig["top_k"].default == 5 and sig["oversample"].default == 4 and sig["metric"].default == "cosine_similarity"
    assert sig["first_metric"].default is None and sig["first_queries"].default is None
    for name in ("rerank_device", "rerank"):
        assert list(inspect.signature(getattr(GpuIndex, name)).parameters) == ["self", "Q", "cand", "k", "metric_id"]
    with pytest.raises(NotImplementedError):
        ranking.rank_two_stage(object(), object(), np.zeros((1, 4)))


def test_rerank_workspace_layout(tmp_path):
    """RerankWs over nq x chunk x m x d x pearson, compiled and run like tests/ws_layout_check.hip: host code under AddressSanitizer
    and UBSan, size equals placement at every point."""
    out = host_check.run(host_check.build("rerank_ws_check", tmp_path))
