"""The selection launchers of hdb_launch.h (hdb_select.hip) bound with ctypes on torch device buffers, for
tests/test_select_kernels.py: histogram passes, the two threshold kernels, collect and finalize, driven directly with score
arrays and candidate lists built for the purpose.

Three rules:
  * cap is always 8192 (HDB_CAND_CAP), the only value the product uses: hdb_launch_finalize raises the kernel's dynamic-LDS
    attribute once per process, from its first call; a smaller first cap would leave later product calls of the same process
    unable to launch;
  * the buffers lie as the product lays them out -- cnt at a stride of 32 words per query, hist [nq][4][256], tie_info 4 words
    per query, a 16-byte aligned score base, ld a multiple of 4 -- and cnt and hist are cleared before each selection, as
    select_exact (hdb_api.hip) does;
  * launches go to the current torch stream and the results are read after a synchronisation.
A missing symbol is an AttributeError: the tests fail, they do not skip.
"""
import ctypes

import numpy as np
import torch

from hyperdb import _native
import select_model as sm

CAP = sm.CAP
CNT_STRIDE = sm.CNT_STRIDE
_vp, _i32, _i64, _u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint32

_SIGNATURES = {
    # (scores, n, ld, nq, hist, pass, k, stream)
    "hdb_launch_hist": [_vp, _i64, _i64, _i32, _vp, _i32, _u32, _vp],
    # (hist, nq, npass, m, sample_n, thr, cnt, stream)
    "hdb_launch_thr": [_vp, _i32, _i32, _u32, _u32, _vp, _vp, _vp],
    # (scores, n, ld, nq, m, thr, cnt, tile_ctr, stream)
    "hdb_launch_sample_thr": [_vp, _i64, _i64, _i32, _u32, _vp, _vp, _vp, _vp],
    # (scores, n, ld, nq, hist, npass, k, cnt, cand, cap, tie_info, stream)
    "hdb_launch_collect": [_vp, _i64, _i64, _i32, _vp, _i32, _u32, _vp, _vp, _u32, _vp, _vp],
    # (cand, cnt, cap, nq, k, kk, row_base, idx_out, score_out, status, qnan, threads, inf_status, stream)
    "hdb_launch_finalize": [_vp, _vp, _u32, _i32, _u32, _u32, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _vp],
}
_bound = {}


def fn(name):
    f = _bound.get(name)
    if f is None:
        f = getattr(_native.lib(), name)              # AttributeError when the library does not export it
        f.argtypes = _SIGNATURES[name]
        f.restype = ctypes.c_int
        _bound[name] = f
    return f


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _launch(name, *args):
    rc = fn(name)(*args)
    assert rc == 0, "%s: launch error %d" % (name, rc)


def _u32_np(t):
    return t.cpu().numpy().view(np.uint32)


def score_buffer(arrays, n):
    """[nq][ld] float32 on the device, ld a multiple of 4 beyond n; the slack scores[q][n:ld] is +inf, so a read past n changes
    the answer."""
    ld = (n + 3) // 4 * 4 + 4
    h = np.full((len(arrays), ld), np.inf, dtype=np.float32)
    for q, a in enumerate(arrays):
        assert a.dtype == np.float32 and a.shape == (n,)
        h[q, :n] = a
    t = torch.from_numpy(h).to(_dev())
    assert t.data_ptr() % 16 == 0
    return t, ld


class Workspace:
    """cnt | hist | tie_info | cand of nq queries, as the product's workspace holds them."""

    def __init__(self, nq):
        d = _dev()
        self.nq = nq
        self.cnt = torch.zeros(nq * CNT_STRIDE, dtype=torch.int32, device=d)
        self.hist = torch.zeros((nq, 4, 256), dtype=torch.int32, device=d)
        self.tie_info = torch.zeros(nq * 4, dtype=torch.int32, device=d)
        self.cand = torch.full((nq, CAP), -1, dtype=torch.int64, device=d)      # (all ones: an entry above every real one)

    def clear(self):
        self.cnt.zero_()
        self.hist.zero_()


def run_finalize(ws, nq, k, kk, row_base=0, qnan=None, threads=1024, inf_status=0):
    """hdb_launch_finalize over ws.cand / ws.cnt -> (idx int64 [nq][k], score bits uint32 [nq][k], status int32 [nq])."""
    d = _dev()
    idx = torch.full((nq, k), -7, dtype=torch.int64, device=d)
    score = torch.full((nq, k), 7.0, dtype=torch.float32, device=d)
    status = torch.full((nq,), -7, dtype=torch.int32, device=d)
    qn = None if qnan is None else torch.tensor(list(qnan), dtype=torch.int32, device=d)
    _launch("hdb_launch_finalize", _p(ws.cand), _p(ws.cnt), CAP, nq, k, kk, row_base, _p(idx), _p(score), _p(status),
            _p(qn) if qn is not None else None, threads, inf_status, _stream())
    torch.cuda.synchronize()
    return idx.cpu().numpy(), _u32_np(score), status.cpu().numpy()


def exact_select(arrays, n, k, npass=4, row_base=0, threads=1024):
    """The exact selection as select_exact + finalize run it: hist x npass, collect, finalize.  -> dict of host arrays: idx,
    bits, status, cnt [nq], tie_info [nq][4] (uint32), cand [nq][CAP] (uint64)."""
    nq = len(arrays)
    kk = min(k, n)
    scores, ld = score_buffer(arrays, n)
    ws = Workspace(nq)
    ws.clear()
    for ps in range(npass):
        _launch("hdb_launch_hist", _p(scores), n, ld, nq, _p(ws.hist), ps, kk, _stream())
    _launch("hdb_launch_collect", _p(scores), n, ld, nq, _p(ws.hist), npass, kk, _p(ws.cnt), _p(ws.cand), CAP, _p(ws.tie_info), _stream())
    idx, bits, status = run_finalize(ws, nq, k, kk, row_base, None, threads, 0)
    return {"idx": idx, "bits": bits, "status": status, "cnt": _u32_np(ws.cnt)[::CNT_STRIDE].copy(),
            "tie_info": _u32_np(ws.tie_info).reshape(nq, 4), "cand": ws.cand.cpu().numpy().view(np.uint64)}


def finalize_lists(lists, totals, k, kk, row_base=0, qnan=None, threads=1024, inf_status=0):
    """Finalize alone over packed candidate lists (uint64 arrays of min(total, CAP) entries each); the rest of each query's
    CAP slots holds all-ones entries, which would sort first if they were read."""
    nq = len(lists)
    ws = Workspace(nq)
    h = np.full((nq, CAP), np.uint64(0xFFFFFFFFFFFFFFFF), dtype=np.uint64)
    c = np.zeros(nq * CNT_STRIDE, dtype=np.uint32)
    for q, (lst, total) in enumerate(zip(lists, totals)):
        assert len(lst) == min(total, CAP)
        h[q, :len(lst)] = lst
        c[q * CNT_STRIDE] = total
    ws.cand.copy_(torch.from_numpy(h.view(np.int64)))
    ws.cnt.copy_(torch.from_numpy(c.view(np.int32)))
    return run_finalize(ws, nq, k, kk, row_base, qnan, threads, inf_status)


def sample_threshold(arrays, n, m, with_tile_ctr):
    """hdb_launch_sample_thr -> (thr bits uint32 [nq], cnt [nq], the tile counter afterwards or None)."""
    nq = len(arrays)
    d = _dev()
    scores, ld = score_buffer(arrays, n)
    thr = torch.full((nq,), 7.0, dtype=torch.float32, device=d)
    cnt = torch.full((nq * CNT_STRIDE,), 77, dtype=torch.int32, device=d)
    ctr = torch.full((1,), 77, dtype=torch.int32, device=d) if with_tile_ctr else None
    _launch("hdb_launch_sample_thr", _p(scores), n, ld, nq, m, _p(thr), _p(cnt), _p(ctr) if ctr is not None else None, _stream())
    torch.cuda.synchronize()
    return _u32_np(thr), _u32_np(cnt)[::CNT_STRIDE].copy(), None if ctr is None else int(ctr.item())


def radix_threshold(arrays, n, m):
    """hist x 4, then hdb_launch_thr -> (thr bits uint32 [nq], cnt [nq])."""
    nq = len(arrays)
    d = _dev()
    scores, ld = score_buffer(arrays, n)
    hist = torch.zeros((nq, 4, 256), dtype=torch.int32, device=d)
    thr = torch.full((nq,), 7.0, dtype=torch.float32, device=d)
    cnt = torch.full((nq * CNT_STRIDE,), 77, dtype=torch.int32, device=d)
    for ps in range(4):
        _launch("hdb_launch_hist", _p(scores), n, ld, nq, _p(hist), ps, m, _stream())
    _launch("hdb_launch_thr", _p(hist), nq, 4, m, n, _p(thr), _p(cnt), _stream())
    torch.cuda.synchronize()
    return _u32_np(thr), _u32_np(cnt)[::CNT_STRIDE].copy()
