"""Host side of the multi-vector queries (hdb_maxsim_host): the ABI, the argument errors that are decided before any HIP call, the
packer of query sets, the numpy model of the contract against a brute-force triple loop, the block / chunk plan and the workspace
(csrc/hdb_maxsim_plan.h, MaxsimWs) and the group keys the facade returns.  No GPU is used."""
import ctypes
import glob
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")


def _err(lib):
    return lib.hdb_last_error().decode()


def test_version_export_and_prototype():
    from hyperdb import _native
    assert _native.lib().hdb_version() >= 111
    assert "hdb_maxsim_host" in _native.EXPORTS and hasattr(_native.lib(), "hdb_maxsim_host")
    header = open(os.path.join(ROOT, "include", "hyperdb_hip.h")).read()
    assert "int hdb_maxsim_host(hdb_index* ix, const void* dev_Q, const int32_t* host_off, int32_t ns, int32_t k, int metric," in header
    for word in ("several GPUs / shards", "hamming / jaccard", "k > 2048", "per-vector weights", "splitting one huge group over teams", "epilogue"):
        assert word in header, word


def test_python_signatures_and_defaults():
    import hyperdb.ranking_algorithm as ranking
    from hyperdb import HyperDB, _native
    from hyperdb._native import GpuIndex
    assert list(inspect.signature(GpuIndex.maxsim).parameters) == ["self", "Q", "offsets", "k", "metric_id"]
    assert list(inspect.signature(_native.pack_query_sets).parameters) == ["x", "d"]
    mh = inspect.signature(_native.maxsim_host).parameters
    assert list(mh)[:7] == ["V", "query_sets", "groups", "k", "metric", "bias", "mask"] and mh["bias"].default is None and mh["mask"].default is None
    rm = inspect.signature(ranking.rank_maxsim).parameters
    assert list(rm) == ["vectors", "query_sets", "groups", "top_k", "metric"]
    assert rm["groups"].default is None and rm["top_k"].default == 5 and rm["metric"].default == "cosine_similarity"
    assert "rank_maxsim" in ranking.__all__
    qm = inspect.signature(HyperDB.query_multi).parameters
    assert list(qm) == ["self", "query_inputs", "group_by", "top_k", "return_similarities", "filters", "metric"]
    assert qm["group_by"].default == "source" and qm["top_k"].default == 5 and qm["return_similarities"].default is True
    assert qm["filters"].default is None and qm["metric"].default == "cosine_similarity"
    # a handle that is not one index on one device is refused before anything else is looked at
    sharded = ranking.ResidentVectors.__new__(ranking.ResidentVectors)
    sharded.index = object()
    with pytest.raises(NotImplementedError, match="one device"):
        ranking.rank_maxsim(sharded, "not even an array")


def test_argument_errors_before_any_hip_call():
    """Sizes are judged first, from the numbers alone -- the offsets are numbers --; then the handle.  A NULL handle is never
    dereferenced and the query pointer never read."""
    from hyperdb import _native
    lib = _native.lib()
    p = ctypes.c_void_p(64)          # a non-null pointer that is never read: every call below fails before it would be
    def call(off, k, ns=None, metric=1, ix=None):
        arr = (ctypes.c_int32 * len(off))(*off) if off is not None else None
        return lib.hdb_maxsim_host(ix, p, arr, len(off) - 1 if ns is None else ns, k, metric, p, None)
    assert call([0, 3], 10, ns=0) == -1 and "ns" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call([0, 3], 10, ns=-2) == -1 and "ns" in _err(lib) and "positive" in _err(lib)
    assert call([0, 3], 0) == -1 and "k must be" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call([0, 3], -4) == -1 and "k must be" in _err(lib)
    assert call([0, 3], 2049) == -3 and "2048" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call(None, 10, ns=1) == -1 and "host_off" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call([1, 3], 10) == -1 and "host_off[0]" in _err(lib) and "got 1" in _err(lib)
    assert call([0, 3, 3, 5], 10) == -1 and "set 1" in _err(lib) and "increasing" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call([0, 3, 2], 10) == -1 and "set 1" in _err(lib)
    assert call([0, 0], 10) == -1 and "set 0" in _err(lib)
    # everything legal in the numbers: the handle fails, the largest k included
    assert call([0, 3], 10) == -1 and "null" in _err(lib) and "hdb_maxsim_host" in _err(lib)
    assert call([0, 1, 5, 10, 19, 52], 2048) == -1 and "null" in _err(lib)
    with pytest.raises(NotImplementedError):
        _native._check(call([0, 3], 5000), "hdb_maxsim_host")
    with pytest.raises(ValueError, match="set 2"):
        _native._check(call([0, 1, 2, 2], 5), "hdb_maxsim_host")


def test_pack_query_sets():
    from hyperdb._native import pack_query_sets
    rng = np.random.default_rng(0)
    a = rng.standard_normal((3, 8))
    flat, off = pack_query_sets(a, 8)                                              # (T, d): one set
    assert flat.dtype == np.float32 and flat.shape == (3, 8) and off.dtype == np.int32 and off.tolist() == [0, 3]
    assert np.array_equal(flat, a.astype(np.float32)) and flat.flags.c_contiguous
    b = rng.standard_normal((4, 2, 8))
    flat, off = pack_query_sets(b, 8)                                              # (S, T, d)
    assert flat.shape == (8, 8) and off.tolist() == [0, 2, 4, 6, 8] and np.array_equal(flat[2:4], b[1].astype(np.float32))
    rag = [rng.standard_normal((t, 8)) for t in (1, 4, 5, 9, 33)]
    flat, off = pack_query_sets(rag, 8)                                            # ragged list
    assert flat.shape == (52, 8) and off.tolist() == [0, 1, 5, 10, 19, 52] and np.array_equal(flat[10:19], rag[3].astype(np.float32))
    with pytest.raises(ValueError, match="set 1 is empty"):
        pack_query_sets([a, np.zeros((0, 8))], 8)
    with pytest.raises(ValueError, match="width 7"):
        pack_query_sets([a, np.zeros((2, 7))], 8)
    with pytest.raises(ValueError, match="width 8"):
        pack_query_sets(a, 16)
    with pytest.raises(ValueError, match="at least one set"):
        pack_query_sets([], 8)
    with pytest.raises(ValueError):
        pack_query_sets(np.zeros(8), 8)
    with pytest.raises(ValueError, match="set 0"):
        pack_query_sets([np.zeros(8)], 8)


def _brute(V, sets, groups, n_groups, k, bias, mask):
    """score(s, g) = sum_t max_{r in g, eligible} (V[r] . q_t + bias[r]), by three loops over Python integers."""
    out_i, out_s = [], []
    for S in sets:
        totals = {}
        for g in range(n_groups):
            total = 0
            for q in S:
                best = None
                for r in range(len(V)):
                    if groups[r] != g or (mask is not None and not mask[r]):
                        continue
                    x = int(sum(int(a) * int(b) for a, b in zip(V[r], q))) + (int(bias[r]) if bias is not None else 0)
                    best = x if best is None or x > best else best
                if best is None:
                    total = None
                    break
                total += best
            if total is not None:
                totals[g] = total
        order = sorted(totals, key=lambda g: (-totals[g], g))[:k]
        out_i.append(order + [-1] * (k - len(order)))
        out_s.append([float(totals[g]) for g in order] + [-np.inf] * (k - len(order)))
    return np.array(out_i, dtype=np.int64), np.array(out_s, dtype=np.float64)


def test_maxsim_host_against_brute_force():
    from hyperdb._native import maxsim_host
    rng = np.random.default_rng(7)
    V = rng.integers(-8, 9, size=(200, 8)).astype(np.float32)
    groups = rng.integers(0, 23, size=200)
    groups[groups == 11] = 12                                                      # group 11 is empty
    n_groups = 25                                                                  # ... and so are 23 and 24
    sets = [rng.integers(-8, 9, size=(t, 8)).astype(np.float32) for t in (1, 3, 2, 6)]   # ragged
    bias = rng.integers(-50, 51, size=200).astype(np.float32)
    mask = rng.random(200) < 0.7
    mask[groups == 4] = False                                                      # a group with every row removed
    for b, m in ((None, None), (bias, None), (None, mask), (bias, mask)):
        for k in (1, 5, 40):                                                       # 40: beyond the groups that exist
            gi, gs = maxsim_host(V, sets, groups, k, "dot_product", bias=b, mask=m, n_groups=n_groups)
            ei, es = _brute(V, sets, groups, n_groups, k, b, m)
            assert gi.dtype == np.int64 and gs.dtype == np.float64 and gi.shape == (4, k)
            assert np.array_equal(gi, ei) and np.array_equal(gs, es), (b is not None, m is not None, k)
            assert not (gi == 11).any() and not (gi >= 23).any()
            if m is not None:
                assert not (gi == 4).any()
    gi, gs = maxsim_host(V, sets, groups, 40, "dot_product", mask=mask, n_groups=n_groups)
    assert (gi[:, -1] == -1).all() and np.isneginf(gs[:, -1]).all()
    # ids outside [0, n_groups) count as masked rows
    bad = groups.copy()
    bad[[3, 77]] = [-5, 90]
    ok = np.ones(200, dtype=bool)
    ok[[3, 77]] = False
    gi, gs = maxsim_host(V, sets, bad, 10, "dot_product", n_groups=n_groups)
    ei, es = maxsim_host(V, sets, groups, 10, "dot_product", mask=ok, n_groups=n_groups)
    assert np.array_equal(gi, ei) and np.array_equal(gs, es)
    with pytest.raises(ValueError, match="one entry per row"):
        maxsim_host(V, sets, groups[:-1], 3, "dot_product")


def test_maxsim_plan_and_workspace(tmp_path):
    """tests/maxsim_plan_check.hip, compiled and run like tests/group_plan_check.hip: host code under AddressSanitizer and UBSan."""
    out = host_check.run(host_check.build("maxsim_plan_check", tmp_path))


def test_workspace_areas_are_declared_once():
    """The areas of the multi-vector call -- acc, the device offsets, the selection's buffers -- are regions of ONE layout in
    hdb_ws.h; no other file of the library takes a region from the workspace, and the call lays that layout out through ws_lay."""
    text = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip"))}
    assert sum(len(re.findall(r"\bstruct MaxsimWs\b", t)) for t in text.values()) == 1 and "struct MaxsimWs" in text["hdb_ws.h"]
    body = text["hdb_ws.h"].split("struct MaxsimWs", 1)[1].split("};", 1)[0]
    for area in ("acc", "voff", "snan", "cnt", "hist", "tie_info", "cand"):
        assert len(re.findall(rf"\b{area} = b\.take<", body)) == 1, area
    assert "TopkWs t;" in body and "t.lay(b," in body
    for name, t in text.items():
        if name != "hdb_ws.h":
            assert ".take<" not in t, f"{name} takes a workspace region outside hdb_ws.h"
    api = text["hdb_api.hip"]
    assert re.search(r"MaxsimWs w;\s*\n\s*rc = ws_lay\(ix, w,", api)
    # the launchers: declared once, in hdb_launch.h
    launch = text["hdb_launch.h"]
    for fn in ("hdb_maxsim_sort_temp_bytes", "hdb_launch_maxsim_keys", "hdb_launch_maxsim_iota", "hdb_launch_maxsim_sort", "hdb_launch_maxsim_offsets",
               "hdb_launch_maxsim_setnan", "hdb_launch_maxsim_reduce"):
        assert len(re.findall(rf"\b{fn}\(", launch)) == 1, fn


def _facade(n_rows, docs, sources, dead=(), metadata_keys=()):
    """A HyperDB whose host lists are set by hand over a stand-in index of n_rows device rows: the key mapping is host code."""
    from hyperdb import HyperDB
    db = HyperDB(metadata_keys=list(metadata_keys))
    db.documents, db.source_indices = list(docs), list(sources)
    db._index = SimpleNamespace(n=n_rows, close=lambda: None)
    db._dead = np.asarray(sorted(dead), dtype=np.int64)
    return db


def test_query_multi_key_mapping_without_gpu():
    docs = [{"name": f"d{i}", "info": {"type": "even" if i % 2 == 0 else "odd"}} for i in range(6)]
    db = _facade(6, docs, [0, 0, 3, 3, 3, 7], metadata_keys=["info.type"])
    codes, ng = db._group_codes("source")
    assert codes.tolist() == [0, 0, 1, 1, 1, 2] and ng == 3
    # groups 1, 2 then the -1 tail: keys are the source_indices entries, members in store order
    res = db._multi_results("source", codes, np.array([1, 2, -1]), np.array([5.0, 4.5, -np.inf]), None, True)
    assert [(k, s) for k, s, _ in res] == [(3, 5.0), (7, 4.5)]
    assert [d["name"] for d in res[0][2]] == ["d2", "d3", "d4"] and [d["name"] for d in res[1][2]] == ["d5"]
    assert db._multi_results("source", codes, np.array([1, 2, -1]), np.array([5.0, 4.5, -np.inf]), None, False) == [3, 7]
    # a filter keeps documents 2 and 4 of group 1 only
    keep = np.array([True, False, True, False, True, True])
    res = db._multi_results("source", codes, np.array([1, 0]), np.array([2.0, 1.0]), keep, True)
    assert [d["name"] for d in res[0][2]] == ["d2", "d4"] and [d["name"] for d in res[1][2]] == ["d0"] and res[1][0] == 0
    # a metadata key: the value is the key; a document without it is a group of its own and is called None
    docs2 = [{"info": {"type": "a"}}, {"name": "no key"}, "a string", {"info": {"type": "a"}}, {"info": {}}, {"info": {"type": "b"}}]
    db2 = _facade(6, docs2, list(range(6)), metadata_keys=["info.type"])
    codes2, ng2 = db2._group_codes("info.type")
    res = db2._multi_results("info.type", codes2, np.array([codes2[0], codes2[2], codes2[5], codes2[1]]), np.array([4.0, 3.0, 2.0, 1.0]), None, True)
    assert [k for k, _, _ in res] == ["a", None, "b", None]
    assert res[0][2] == [docs2[0], docs2[3]] and res[1][2] == ["a string"] and res[3][2] == [docs2[1]]
    # tombstones: 8 device rows, rows 2 and 5 dead, the six documents sit on the live rows in order
    db3 = _facade(8, docs, [0, 0, 1, 1, 2, 2], dead=(2, 5))
    codes3, ng3 = db3._group_codes("source")
    res = db3._multi_results("source", codes3, np.array([2, 0, 1]), np.array([3.0, 2.0, 1.0]), None, True)
    assert [k for k, _, _ in res] == [2, 0, 1] and [d["name"] for d in res[0][2]] == ["d4", "d5"] and [d["name"] for d in res[1][2]] == ["d0", "d1"]
    for d in (db, db2, db3):
        d._index = None                                # (nothing for __del__ paths to close)
