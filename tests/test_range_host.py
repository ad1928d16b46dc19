"""Host side of the range search (hdb_range_host, hdb_range_fetch): the ABI, the plan of a call (csrc/hdb_range_plan.h), the numpy model
of the contract against a brute-force loop, and the argument errors.  No GPU is used."""
import ctypes

import numpy as np
import pytest

import host_check


def test_version_and_exports():
    from hyperdb import _native
    assert _native.lib().hdb_version() >= 113
    for name in ("hdb_range_host", "hdb_range_fetch"):
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)


def test_plan_over_a_grid(tmp_path):
    host_check.run(host_check.build("range_plan_check", tmp_path))


@pytest.mark.parametrize("sort", [True, False])
def test_the_model_against_a_loop(sort):
    """Six rows, dot product: row 0 meets the threshold of query 0 exactly, row 1 is masked, row 2 scores NaN, rows 3 and 4 tie at 5
    after the bias, row 5 is the best; query 1's threshold is above everything."""
    from hyperdb._native import range_host
    V = np.array([[3.0, 0], [8, 0], [np.nan, 0], [4, 0], [5, 0], [9, 0]])
    Q = np.array([[1.0, 0], [1.0, 0]])
    bias = np.array([0.0, 0, 0, 1, 0, 0])
    mask = np.array([1, 0, 1, 1, 1, 1])
    thr = [3.0, 100.0]
    lims, idx, sc = range_host(V, Q, thr, "dot_product", bias=bias, mask=mask, sort=sort)
    want_i, want_s, want_l = [], [], [0]
    for q in range(2):
        s = [float(V[r] @ Q[q]) + bias[r] for r in range(6)]
        hits = sorted(((-s[r], r) if sort else (r, r)) for r in range(6) if mask[r] and s[r] >= np.float32(thr[q]) and s[r] > -np.inf)
        want_i += [r for _, r in hits]
        want_s += [s[r] for _, r in hits]
        want_l.append(len(want_i))
    assert want_i == ([5, 3, 4, 0] if sort else [0, 3, 4, 5]) and want_l == [0, 4, 4]       # (the case is what the docstring says)
    assert lims.tolist() == want_l and idx.tolist() == want_i and sc.tolist() == want_s
    assert lims.dtype == np.int64 and idx.dtype == np.int64 and sc.dtype == np.float64


def test_argument_errors():
    """NaN and +inf thresholds and a wrong threshold count: ValueError in the model, HDB_ERR_ARG from the library before the handle
    is looked at (NULL here); hamming / jaccard are not built; a fetch without a handle is refused."""
    from hyperdb import _native
    lib = _native.lib()
    V, Q = np.eye(3), np.eye(3)[:2]
    for thr in (np.nan, np.inf, [0.5, np.nan], [0.5], [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError):
            _native.range_host(V, Q, thr, "dot_product")
    with pytest.raises(NotImplementedError):
        _native.range_host(V, Q, 0.5, "hamming_distance")
    assert _native.range_host(np.zeros((0, 3)), Q, 0.5, "dot_product")[0].tolist() == [0, 0, 0]      # n == 0: empty lists
    lims = (ctypes.c_int64 * 3)()
    for bad in (float("nan"), float("inf")):
        thr = (ctypes.c_float * 2)(0.5, bad)
        assert lib.hdb_range_host(None, None, 2, thr, 0, 1, lims, None) == -1
        assert b"query 1" in lib.hdb_last_error()
    assert lib.hdb_range_host(None, None, 2, (ctypes.c_float * 2)(0.5, float("-inf")), 0, 1, lims, None) == -1
    assert b"null index" in lib.hdb_last_error()
    assert lib.hdb_range_host(None, None, -1, None, 0, 1, lims, None) == -1 and lib.hdb_range_fetch(None, None, None) == -1
