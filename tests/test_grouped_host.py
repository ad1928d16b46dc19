"""Host side of the grouped top-k (hdb_index_set_groups, hdb_topk_grouped_host, hdb_collapse_groups): the ABI, the argument errors
that are decided before any HIP call, the group-id check of the Python binding, the numpy model of the collapse, the schedule and
workspace of the call (csrc/hdb_group_plan.h, TopkWs) and the codes the facade builds for group_by.  No GPU is used."""
import ctypes
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hdb_index_set_groups", "hdb_topk_grouped_host", "hdb_collapse_groups")


def _err(lib):
    return lib.hdb_last_error().decode()


def test_version_exports_and_status_bit():
    from hyperdb import _native
    assert _native.lib().hdb_version() >= 110
    for name in NAMES:
        assert name in _native.EXPORTS and hasattr(_native.lib(), name)
    assert _native.Q_GROUPS_SHORT == 16
    header = open(os.path.join(ROOT, "include", "hyperdb_hip.h")).read()
    assert "HDB_Q_GROUPS_SHORT = 16" in header
    for name in NAMES:
        assert f"int {name}(" in header


def test_python_signatures_and_defaults():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb import HyperDB, _native
    from hyperdb._native import GpuIndex
    sig = inspect.signature(ranking.rank_grouped).parameters
    assert list(sig) == ["vectors", "query_vectors", "groups", "top_k", "metric", "timestamps", "recency_bias"]
    assert sig["top_k"].default == 5 and sig["metric"].default == "cosine_similarity"
    assert sig["timestamps"].default is None and sig["recency_bias"].default == 0
    assert "rank_grouped" in ranking.__all__
    s = inspect.signature(GpuIndex.set_groups).parameters
    assert list(s) == ["self", "groups", "n_groups"] and s["n_groups"].default is None
    assert list(inspect.signature(GpuIndex.topk_grouped).parameters) == ["self", "Q", "k", "metric_id"]
    assert list(inspect.signature(_native.collapse_groups).parameters)[:4] == ["idx", "scores", "groups", "k"]
    assert list(inspect.signature(_native.collapse_groups_host).parameters)[:4] == ["idx", "scores", "groups", "k"]
    qb = inspect.signature(HyperDB.query_batch).parameters
    assert list(qb)[-1] == "group_by" and qb["group_by"].default is None
    qg = inspect.signature(HyperDB.query_grouped).parameters
    assert list(qg)[:3] == ["self", "query_input", "group_by"] and qg["top_k"].default == 5
    # group_by is part of the cache key, and None is the ungrouped key exactly
    q = np.array([1.0, 2.0])
    k0 = HyperDB._hashable_key(q, 5, True, None, 0, None, "dot_product", 5)
    assert HyperDB._hashable_key(q, 5, True, None, 0, None, "dot_product", 5, None) == k0
    ks = HyperDB._hashable_key(q, 5, True, None, 0, None, "dot_product", 5, "source")
    assert ks != k0 and ks != HyperDB._hashable_key(q, 5, True, None, 0, None, "dot_product", 5, "info.type") and hash(ks) is not None
    # a handle that is not one index on one device is refused before anything else is looked at
    sharded = ranking.ResidentVectors.__new__(ranking.ResidentVectors)
    sharded.index = object()
    with pytest.raises(NotImplementedError, match="one device"):
        ranking.rank_grouped(sharded, np.zeros((1, 4)), [0])


def test_argument_errors_before_any_hip_call():
    """Sizes are judged first, from the numbers alone; then the handle.  A NULL handle is never dereferenced."""
    from hyperdb import _native
    lib = _native.lib()
    p = ctypes.c_void_p(64)          # a non-null pointer that is never read: every call below fails before it would be
    grouped = lambda ix, nq, k, metric=1: lib.hdb_topk_grouped_host(ix, p, nq, k, metric, p, None)
    collapse = lambda nq, m, k, idx=p, groups=p, n_groups=10, n=100: lib.hdb_collapse_groups(idx, p, nq, m, k, groups, n_groups, n, 0, p, p, p, 0, None)
    # hdb_topk_grouped_host
    assert grouped(None, 2, 10) == -1 and "null" in _err(lib) and "hdb_topk_grouped_host" in _err(lib)
    assert grouped(None, 2, 0) == -1 and "k must be" in _err(lib) and "hdb_topk_grouped_host" in _err(lib)
    assert grouped(None, 2, -3) == -1 and "hdb_topk_grouped_host" in _err(lib)
    assert grouped(None, 2, 2049) == -3 and "2048" in _err(lib) and "hdb_topk_grouped_host" in _err(lib)
    assert grouped(None, 2, 2048) == -1 and "null" in _err(lib)                 # the largest k passes the size check: the handle fails
    assert grouped(None, -1, 10) == -1 and "nq" in _err(lib) and "hdb_topk_grouped_host" in _err(lib)
    assert grouped(None, 0, 10) == -1 and "positive" in _err(lib)
    # hdb_collapse_groups
    assert collapse(2, 100, 10, idx=None) == -1 and "null" in _err(lib) and "hdb_collapse_groups" in _err(lib)
    assert collapse(2, 100, 10, groups=None) == -1 and "null" in _err(lib)
    for m, k, word in ((0, 1, "[1, 2048]"), (2049, 10, "[1, 2048]"), (-5, 1, "[1, 2048]"), (100, 101, "[1, m]"), (100, 0, "[1, m]"), (1, 2, "[1, m]")):
        assert collapse(2, m, k, idx=None) == -1, (m, k)
        assert word in _err(lib) and "hdb_collapse_groups" in _err(lib), (m, k, _err(lib))
    assert collapse(-1, 100, 10) == -1 and "nq" in _err(lib) and "hdb_collapse_groups" in _err(lib)
    assert collapse(2, 100, 10, n_groups=0) == -1 and "n_groups" in _err(lib)
    assert collapse(0, 100, 10, idx=None) == 0                                   # no query: nothing to do
    assert collapse(2, 2048, 2048, idx=None) == -1 and "null" in _err(lib)       # the largest list and k = m pass the size check
    # hdb_index_set_groups
    assert lib.hdb_index_set_groups(None, p, 5) == -1 and "null index" in _err(lib) and "hdb_index_set_groups" in _err(lib)
    with pytest.raises(NotImplementedError):
        _native._check(grouped(None, 1, 5000), "hdb_topk_grouped_host")


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_group_id_validation(kind):
    from hyperdb._native import check_groups
    mk = (lambda a, dt=np.int64: np.asarray(a, dtype=dt)) if kind == "numpy" else (lambda a, dt=np.int64: torch.from_numpy(np.asarray(a, dtype=dt)))
    g, top = check_groups(mk([0, 2, 2, 1, 5]), 5)
    assert top == 6 and g.dtype == torch.int32 and g.tolist() == [0, 2, 2, 1, 5]
    for dt in (np.int8, np.int16, np.int32, np.uint8):
        assert check_groups(mk([3, 0, 1], dt), 3)[1] == 4
    with pytest.raises(ValueError, match="one entry per row"):
        check_groups(mk([0, 1, 2]), 4)                                            # wrong length
    with pytest.raises(ValueError, match="one entry per row"):
        check_groups(mk([[0, 1], [2, 3]]), 4)                                     # not 1-D
    with pytest.raises(ValueError, match="-1"):
        check_groups(mk([0, -1, 2]), 3)                                           # a negative id, named
    with pytest.raises(ValueError, match="integers"):
        check_groups(mk([0.0, 1.0, 2.0], np.float32), 3)                          # float dtype
    with pytest.raises(ValueError, match="integers"):
        check_groups(mk([True, False, True], np.bool_), 3)
    # the cache of arrays that passed: a tensor that is already what the device wants is returned as it is, the second time unread
    from collections import OrderedDict
    seen = OrderedDict()
    t = torch.tensor([1, 0, 1], dtype=torch.int32)
    g1, top1 = check_groups(t, 3, seen, None)
    assert g1 is t and top1 == 2
    seen[id(g1)] = (g1, top1)
    t[1] = -7                                                                      # (not looked at again: one check per array)
    assert check_groups(t, 3, seen, None) == (t, 2)


def test_set_groups_n_groups_too_small_names_the_value():
    """GpuIndex.set_groups without a GPU: the host checks run before anything touches the handle."""
    from hyperdb._native import GpuIndex
    from collections import OrderedDict
    ix = GpuIndex.__new__(GpuIndex)
    ix.n, ix.device, ix._groups_ok, ix._groups, ix.n_groups = 4, None, OrderedDict(), None, 0
    ix._h = ctypes.c_void_p()                                                      # (close() of the unbuilt object: nothing to destroy)
    ix._host_records, ix._qstage, ix._buf = OrderedDict(), OrderedDict(), None
    with pytest.raises(ValueError, match=r"group id 7 is not in \[0, 5\)"):
        ix.set_groups(np.array([0, 7, 1, 2]), n_groups=5)
    with pytest.raises(ValueError, match="one entry per row"):
        ix.set_groups(np.array([0, 1, 2]))
    with pytest.raises(ValueError, match="-1"):
        ix.set_groups(torch.tensor([0, 1, -1, 2]))
    with pytest.raises(ValueError, match="integers"):
        ix.set_groups(np.array([0.0, 1.0, 2.0, 3.0]))
    ix.set_groups(None)                                                            # nothing set: nothing to clear, no C call
    assert ix._groups is None and ix.n_groups == 0


def test_collapse_groups_host_on_hand_written_lists():
    from hyperdb._native import collapse_groups_host, Q_BADROW, Q_GROUPS_SHORT
    groups = np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4])                              # rows 2g, 2g + 1 form group g
    sc = lambda *v: np.array([v], dtype=np.float32)
    # repeats: rows 1 and 0 share group 0, rows 4 and 5 group 2
    i, s, st = collapse_groups_host(np.array([[1, 0, 4, 5, 9, 2]]), sc(9, 8, 7, 6, 5, 4), groups, 3)
    assert i.tolist() == [[1, 4, 9]] and s.tolist() == [[9, 7, 5]] and st.tolist() == [0]
    # the same list, k = 4: the fourth group is row 2's
    i, s, st = collapse_groups_host(np.array([[1, 0, 4, 5, 9, 2]]), sc(9, 8, 7, 6, 5, 4), groups, 4)
    assert i.tolist() == [[1, 4, 9, 2]] and st.tolist() == [0]
    # k = 5 of a list of 6 < n rows with only 4 groups and no padding: short, and the list was not exhaustive
    i, s, st = collapse_groups_host(np.array([[1, 0, 4, 5, 9, 2]]), sc(9, 8, 7, 6, 5, 4), groups, 5)
    assert i.tolist() == [[1, 4, 9, 2, -1]] and s[0, 4] == -np.inf and st.tolist() == [Q_GROUPS_SHORT]
    # a -1 tail: the list is exhaustive, a short answer is the whole answer
    i, s, st = collapse_groups_host(np.array([[3, 2, 7, -1, -1, -1]]), sc(5, 4, 3, -np.inf, -np.inf, -np.inf), groups, 3)
    assert i.tolist() == [[3, 7, -1]] and s.tolist() == [[5, 3, -np.inf]] and st.tolist() == [0]
    # an entry at -inf is padding too (an excluded row an exact selection handed out)
    i, s, st = collapse_groups_host(np.array([[3, 8, 6]]), sc(5, 4, -np.inf), groups, 3)
    assert i.tolist() == [[3, 8, -1]] and st.tolist() == [0]
    # all one group
    i, s, st = collapse_groups_host(np.array([[5, 4, 5, 4]]), sc(4, 3, 2, 1), groups, 2)
    assert i.tolist() == [[5, -1]] and st.tolist() == [Q_GROUPS_SHORT]
    one = np.zeros(4, dtype=np.int64)
    i, s, st = collapse_groups_host(np.array([[3, 1, 0, 2]]), sc(4, 3, 2, 1), one, 2)
    assert i.tolist() == [[3, -1]] and st.tolist() == [0]                         # m = n: the whole ranking, never short
    # all distinct, k = m
    i, s, st = collapse_groups_host(np.array([[8, 0, 2, 5]]), sc(4, 3, 2, 1), groups, 4)
    assert i.tolist() == [[8, 0, 2, 5]] and s.tolist() == [[4, 3, 2, 1]] and st.tolist() == [0]
    # ids outside the index are skipped and flagged; a row base shifts the ids
    i, s, st = collapse_groups_host(np.array([[108, 99, 110, 103, 102]]), sc(5, 4, 3, 2, 1), groups, 2, row_base=100)
    assert i.tolist() == [[108, 103]] and st.tolist() == [Q_BADROW]
    # several queries at once
    i, s, st = collapse_groups_host(np.array([[0, 1, 2], [9, 8, -1]]), np.array([[3, 2, 1], [3, 2, -np.inf]], np.float32), groups, 2)
    assert i.tolist() == [[0, 2], [9, -1]] and st.tolist() == [0, 0]


def test_group_plan_and_workspace(tmp_path):
    """tests/group_plan_check.hip, compiled and run like tests/rerank_ws_check.hip: host code under AddressSanitizer and UBSan.  The
    round schedule over (n, k, oversample, rounds), the exact plan over shapes, dtypes and metrics, size equals placement."""
    out = host_check.run(host_check.build("group_plan_check", tmp_path))


def _facade(n_rows, docs, sources, dead=(), metadata_keys=()):
    """A HyperDB whose host lists are set by hand over a stand-in index of n_rows device rows: _group_codes is host code."""
    from hyperdb import HyperDB
    db = HyperDB(metadata_keys=list(metadata_keys))
    db.documents, db.source_indices = list(docs), list(sources)
    db._index = SimpleNamespace(n=n_rows, close=lambda: None)
    db._dead = np.asarray(sorted(dead), dtype=np.int64)
    return db


def test_facade_group_codes_without_gpu():
    docs = [{"name": f"d{i}", "info": {"type": "even" if i % 2 == 0 else "odd"}} for i in range(6)]
    # source: documents of one source share a code, codes are dense
    db = _facade(6, docs, [0, 0, 3, 3, 3, 7], metadata_keys=["info.type"])
    rows, ng = db._group_codes("source")
    assert rows.dtype == np.int32 and rows.tolist() == [0, 0, 1, 1, 1, 2] and ng == 3
    # a metadata key: one code per value
    rows, ng = db._group_codes("info.type")
    assert rows.tolist() == [0, 1, 0, 1, 0, 1] and ng == 2
    # documents that lack the key -- or are no dict -- are each their own group
    docs2 = [{"info": {"type": "a"}}, {"name": "no key"}, "a string", {"info": {"type": "a"}}, {"info": {}}, {"info": {"type": "b"}}]
    db = _facade(6, docs2, list(range(6)), metadata_keys=["info.type"])
    rows, ng = db._group_codes("info.type")
    assert rows[0] == rows[3] and len({int(rows[i]) for i in (0, 1, 2, 4, 5)}) == 5 and ng == 5
    assert rows.min() == 0 and rows.max() == ng - 1
    # after a removal that leaves tombstones: 8 device rows, rows 2 and 5 dead, the six documents sit on the live rows in order;
    # a dead row holds a valid code (it is masked)
    db = _facade(8, docs, [0, 0, 1, 1, 2, 2], dead=(2, 5), metadata_keys=["info.type"])
    rows, ng = db._group_codes("source")
    assert ng == 3 and rows[[0, 1, 3, 4, 6, 7]].tolist() == [0, 0, 1, 1, 2, 2]
    assert 0 <= rows[2] < ng and 0 <= rows[5] < ng
    rows, ng = db._group_codes("info.type")
    assert rows[[0, 1, 3, 4, 6, 7]].tolist() == [0, 1, 0, 1, 0, 1] and 0 <= rows[2] < ng
    # anything else is refused by name
    for bad in ("colour", "name", 5, ""):
        with pytest.raises(ValueError, match="group_by"):
            db._group_codes(bad)
    with pytest.raises(ValueError, match="source_indices"):
        _facade(6, docs, [0, 1])._group_codes("source")
    db._index = None                                  # (nothing for __del__ paths to close)
