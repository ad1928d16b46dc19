"""MI355X-native drop-in for the reference's ``hyperdb/ranking_algorithm.py``.

Same public names and signatures as the reference module (``get_norm_vector``, ``dot_product``,
``cosine_similarity``, ``euclidean_metric``, ``hamming_distance``, ``check_and_binarize_vectors``,
``hyperDB_ranking_algorithm_sort``; reference ranking_algorithm.py:8,24,32,44,116,128,149), so
``import hyperdb.ranking_algorithm as ranking`` (reference hyperdb.py:13) keeps working.  The
arithmetic runs in hand-written HIP kernels on gfx950 through the C ABI in
``include/hyperdb_hip.h``; this file only validates arguments, moves data and restores the
reference's return types (int64 indices, float64 scores, ValueError on NaN / unknown metric).

``vectors`` may be, in every function:
  * a numpy array / list of rows  - uploaded for the call (PCIe-inclusive, like a cold start);
  * a CUDA ``torch.Tensor``       - borrowed in place, row caches built per call;
  * a :class:`ResidentVectors`    - registered once with :func:`register_vectors`; the N x d
    matrix and its 1/||v|| cache stay in HBM between calls (what ``HyperDB`` uses).

Additive surface (the reference has no batched call): :func:`rank_batch`; every query against its own list of rows:
:func:`rerank_batch`; a cheap index in front of an exact one in one call: :func:`rank_two_stage`; one hit per group of rows (a
document's chunks): :func:`rank_grouped`; a diverse top-k (maximal marginal relevance): :func:`rank_mmr`.

There is NO CPU fallback: without the HIP library importing this module fails, and without a GPU every
call raises ``HyperDBNativeError`` instead of silently computing on the host.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _native
from ._native import GpuIndex, METRIC_IDS, NAN_MESSAGE, pack_query_sets
from .group import GpuGroup

__all__ = [
    "get_norm_vector", "dot_product", "cosine_similarity", "euclidean_metric", "manhattan_distance",
    "jaccard_similarity", "pearson_correlation", "check_and_binarize_vectors", "hamming_distance",
    "hyperDB_ranking_algorithm_sort", "rank_batch", "register_vectors", "ResidentVectors",
    "rerank_batch", "rank_two_stage", "rank_grouped", "rank_maxsim", "rank_mmr",
]

_GPU_METRICS = tuple(METRIC_IDS)      # all seven metrics of the reference's dispatch table have kernels
_ALL_METRICS = tuple(METRIC_IDS)


class ResidentVectors:
    """Handle for a matrix registered on the GPU; pass it wherever ``vectors`` is expected."""

    def __init__(self, vectors, device=None, devices=None, quantize=None, storage=None, bitorder="big"):
        _native.quant_mode(quantize)                     # (ValueError before anything is uploaded)
        if _native.storage_mode(storage) == "bits" and devices:
            raise NotImplementedError(_native.BITS_SINGLE_INDEX)
        self.index = (GpuGroup(vectors, devices, storage=storage) if devices
                      else GpuIndex(vectors, device=device, storage=storage, bitorder=bitorder))
        if quantize is not None:
            _native.request_shadow(self.index, quantize)     # (a bfloat16 matrix: sets bf16_quant first)
        arr_dtype = vectors.dtype if hasattr(vectors, "dtype") else None
        if storage in ("int8", "bits"):
            arr_dtype = None                             # the STORED dtype decides: an int8 / packed-bit index answers in float32
        self.np_dtype = _np_dtype_of(arr_dtype, self.index)

    @property
    def shape(self):
        return (self.index.n, self.index.d)

    def __len__(self):
        return self.index.n

    def close(self):
        self.index.close()


def register_vectors(vectors, device=None, devices=None, quantize=None, storage=None, bitorder="big"):
    """Upload ``vectors`` once; returns a handle usable in place of ``vectors``.  ``devices=[...]`` row-shards the matrix
    over several GPUs behind the same handle (single process, see hyperdb/group.py).  ``quantize="int8"`` also keeps an int8
    shadow of the matrix that 1-4-query dot / cosine / euclidean calls scan first, rescoring the surviving rows exactly (same
    answer, fewer bytes read; see GpuIndex.quantize).  ``storage="int8"`` keeps the matrix as signed 8-bit integers, one byte per
    element: np.int8 / torch.int8 go in as they are, any other numeric input only if every element is an integer in
    [-128, 127] (ValueError otherwise); queries and scores are float32.  Without it integer inputs are widened to float64.
    ``storage="bits"`` (one device only) keeps a packed-bit matrix, one bit per element: a 2-D uint8 array of packed rows
    ``[n, d/8]`` (``np.packbits`` order; see ``_native.pack_bits``) or a 2-D bool array ``[n, d]``; every metric is the reference's
    arithmetic on the 0/1 matrix the bits stand for, with float32 queries of d elements and float32 scores.  ``bitorder``
    ("big", np.packbits' default, or "little") names the order of the packed bytes; a uint8 query of d/8 bytes is taken as packed
    in the same order."""
    return ResidentVectors(vectors, device=device, devices=devices, quantize=quantize, storage=storage, bitorder=bitorder)


# (bfloat16 has no numpy dtype: score vectors of a bf16 matrix come back as float32, the type its values widen to exactly)
# (float8 e4m3 likewise)
_TORCH2NP = {torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64, torch.bfloat16: np.float32,
             torch.float8_e4m3fn: np.float32}
# ... of a STORED matrix: an int8 index (storage="int8") answers in float32.  Not part of _TORCH2NP, which also reads the dtype of
# raw inputs: a raw torch.int8 tensor handed to a metric function becomes a float64 index and answers in float64
_STORED2NP = dict(_TORCH2NP)
_STORED2NP[torch.int8] = np.float32
_STORED2NP[torch.uint8] = np.float32                 # a packed-bit index (storage="bits"): the 0/1 matrix answers in float32


def _np_dtype_of(dt, index):
    if isinstance(dt, torch.dtype):
        return np.dtype(_TORCH2NP.get(dt, np.float64))
    if dt is not None:
        d = np.dtype(dt)
        return d
    return np.dtype(_STORED2NP[(index.shards[0] if isinstance(index, GpuGroup) else index).V.dtype])


def _resolve(vectors):
    """-> (GpuIndex, numpy dtype of the caller's data, owned flag)."""
    if isinstance(vectors, ResidentVectors):
        return vectors.index, vectors.np_dtype, False
    if isinstance(vectors, GpuIndex):
        return vectors, np.dtype(_STORED2NP[vectors.V.dtype]), False
    if isinstance(vectors, GpuGroup):
        return vectors, np.dtype(_STORED2NP[vectors.shards[0].V.dtype]), False
    if isinstance(vectors, torch.Tensor):
        ix = GpuIndex(vectors)
        return ix, np.dtype(_TORCH2NP.get(vectors.dtype, np.float64)), True
    arr = np.asarray(vectors)
    ix = GpuIndex(arr)
    return ix, arr.dtype, True


def _packed_query(vectors, query_vector):
    """Is this a packed uint8 query of a bits index (storage="bits")?  Such a query is bytes, not elements: never binarised in place."""
    ix = vectors.index if isinstance(vectors, ResidentVectors) else vectors
    return (isinstance(ix, GpuIndex) and ix.dtype == _native.HDB_B1 and isinstance(query_vector, np.ndarray)
            and query_vector.dtype == np.uint8 and query_vector.shape[-1] == ix.d // 8)


def _query_host(query_vector):
    if isinstance(query_vector, torch.Tensor):
        return query_vector.detach().cpu().numpy()
    return np.asarray(query_vector)


def _result_dtype(vdt, q):
    qdt = q.dtype if isinstance(q, np.ndarray) else np.asarray(q).dtype
    try:
        return np.result_type(vdt, qdt)
    except TypeError:
        return np.dtype(np.float64)


def _scores(vectors, query_vector, metric_id, out_dtype=None):
    ix, vdt, owned = _resolve(vectors)
    try:
        qh = _query_host(query_vector)
        s = ix.scores(qh, metric_id).cpu().numpy()
        if out_dtype is None:
            out_dtype = _result_dtype(vdt, qh)
            if not np.issubdtype(out_dtype, np.floating):
                out_dtype = np.dtype(np.float64)
        return s.astype(out_dtype)
    finally:
        if owned:
            ix.close()


# ---------------------------------------------------------------------------------------------
# per-metric functions (reference ranking_algorithm.py:8-147)
# ---------------------------------------------------------------------------------------------
def get_norm_vector(vector):
    """vector / ||vector|| along the last axis, zero norm -> divide by 1 (reference :8-21).

    Host helper: the reference calls it on ONE vector (the ANN query, hyperdb.py:207,:1361); the
    resident matrix never goes through it - its 1/||v|| cache is built on the GPU at registration.
    """
    vector = np.asarray(vector)
    norms = np.linalg.norm(vector, axis=-1, keepdims=True)
    norms = np.where(norms == 0, 1, norms)
    if np.isnan(vector).any():
        print(f"Warning: Vectors at indices {np.where(np.isnan(vector))} contain NaN values.")
    return vector / norms


def dot_product(vectors, query_vector):
    """V . q for every row (reference :24-30) on the GPU; returns an (N,) numpy array."""
    return _scores(vectors, query_vector, METRIC_IDS["dot_product"])


def cosine_similarity(vectors, query_vector):
    """cos(v, q) for every row, zero-norm rows score 0 (reference :32-42)."""
    return _scores(vectors, query_vector, METRIC_IDS["cosine_similarity"])


def euclidean_metric(vectors, query_vector, get_similarity_score=True):
    """1/(1+||v-q||) per row, or the raw distance (reference :44-52)."""
    mid = METRIC_IDS["euclidean_metric"] if get_similarity_score else _native.EUCLIDEAN_DIST
    return _scores(vectors, query_vector, mid)


def check_and_binarize_vectors(vectors):
    """x > 0 -> 1 else 0, IN PLACE unless already binary (reference :116-126).  Host helper used
    to reproduce the reference's visible side effect on the caller's query array."""
    # (the reference asks np.unique for exactly the value sets [0, 1], [0], [1]: "every element is 0 or 1", without the sort)
    if isinstance(vectors, np.ndarray) and vectors.size and bool(((vectors == 0) | (vectors == 1)).all()):
        return vectors
    if not isinstance(vectors, np.ndarray):
        unique_values = np.unique(vectors)
        if any(np.array_equal(unique_values, ok) for ok in ([0, 1], [0], [1])):
            return vectors
    if isinstance(vectors, np.ndarray) and vectors.dtype.kind == "f":
        # the reference's two masked assignments (x > 0 -> 1, x <= 0 -> 0; a NaN is neither and stays) in one masked copy
        np.copyto(vectors, vectors > 0, casting="unsafe", where=(vectors == vectors))
        return vectors
    vectors[vectors > 0] = 1
    vectors[vectors <= 0] = 0
    return vectors


def hamming_distance(vectors, query_vector):
    """d - popcount(sign(v) xor sign(q)) per row as unsigned integers (reference :128-147).

    Like the reference, a numpy ``query_vector`` is binarised in place."""
    out = _scores(vectors, query_vector, METRIC_IDS["hamming_distance"], out_dtype=np.uint64)
    if isinstance(query_vector, np.ndarray) and query_vector.flags.writeable and not _packed_query(vectors, query_vector):
        check_and_binarize_vectors(query_vector)
    return out


def manhattan_distance(vectors, query_vector):
    """1/(1+sum|v-q|) per row (reference :54-61)."""
    return _scores(vectors, query_vector, METRIC_IDS["manhattan_distance"])


def jaccard_similarity(vectors, query_vector):
    """|v AND q| / |v OR q| on the x>0 bits, NaN where both are empty (reference :63-75); float64 like numpy's
    true division.  A numpy ``query_vector`` is binarised in place, as in the reference."""
    out = _scores(vectors, query_vector, METRIC_IDS["jaccard_similarity"], out_dtype=np.float64)
    if isinstance(query_vector, np.ndarray) and query_vector.flags.writeable and not _packed_query(vectors, query_vector):
        check_and_binarize_vectors(query_vector)
    return out


def pearson_correlation(vectors, query_vector):
    """Pearson r per row, NaN when the row or the query is constant (reference :77-113); float64."""
    return _scores(vectors, np.asarray(_query_host(query_vector)).reshape(-1), METRIC_IDS["pearson_correlation"],
                   out_dtype=np.float64)


# ---------------------------------------------------------------------------------------------
# the sort entry (reference ranking_algorithm.py:149-204)
# ---------------------------------------------------------------------------------------------
def _validate_metric(metric):
    if metric not in _ALL_METRICS:
        raise ValueError(f"Unknown metric: {metric}")            # reference :166



def _apply_recency(ix, timestamps, recency_bias):
    """reference :180-183: zeros unless timestamps are given and non-empty."""
    if timestamps is not None and len(timestamps) > 0:
        ix.set_recency(timestamps, recency_bias)
        return True
    ix.set_bias(None)
    return False


def hyperDB_ranking_algorithm_sort(vectors, query_vector, top_k=5, metric='cosine_similarity', timestamps=None,
                                   recency_bias=0):
    """Top-k rows of ``vectors`` for one query (reference ranking_algorithm.py:149-204).

    Returns ``(indices int64 (k,), scores float64 (k,))`` sorted by score descending, ties by index
    ascending.  Behaviour kept from the reference: NaN anywhere -> ValueError (:150-151); unknown
    metric -> ValueError (:166); one stored row -> ``(array([0]), array([[s]]))`` and an Info line
    (:189-191); ``top_k == 0`` -> ``([], [])`` (:202); ``top_k > N`` -> all N rows; hamming binarises
    a numpy query in place (:123-124).
    """
    ix, _, owned = _resolve(vectors)
    try:
        # a CUDA tensor query stays on the device (its NaN check is the kernels' status word, which ix.topk turns into the
        # same ValueError); a host query is checked here and staged once in a pinned buffer by the index
        on_device = isinstance(query_vector, torch.Tensor) and query_vector.is_cuda and ix.n > 1
        qh = query_vector.detach() if on_device else _query_host(query_vector)
        # (one host query: a NaN anywhere makes q.q a NaN -- a dot product instead of an isnan pass and a reduction)
        if ix.has_nan or (not on_device and (math.isnan(float(np.dot(qh, qh))) if (qh.ndim == 1 and qh.dtype.char in "fd") else np.isnan(qh).any())):
            raise ValueError(NAN_MESSAGE)
        _validate_metric(metric)
        if ix.n == 0:
            raise ValueError("vectors is empty")
        had_bias = _apply_recency(ix, timestamps, recency_bias)
        try:
            if ix.n == 1:
                s = ix.scores(qh, METRIC_IDS[metric]).cpu().numpy().astype(np.float64)
                if had_bias:
                    s = s + ix._bias.cpu().numpy().astype(np.float64)
                s[np.isnan(s)] = -np.inf
                print("Info: Only one document left.")
                return np.array([0]), np.array([s])
            k = max(0, min(int(top_k), ix.n))
            if k == 0:
                return [], []
            # views of the index's pinned result record: converted once into the arrays handed back (int64 / float64 like the reference)
            idx_v, sc_v, st_v = ix.topk_views(qh.reshape(1, -1), k, METRIC_IDS[metric])
            if st_v[0] & _native.Q_NAN:
                raise ValueError(NAN_MESSAGE)
            idx, sc = idx_v[0].copy(), sc_v[0].astype(np.float64)
        finally:
            if had_bias:
                ix.set_bias(None)
        if metric in ("hamming_distance", "jaccard_similarity") and isinstance(query_vector, np.ndarray) \
                and query_vector.flags.writeable and not _packed_query(ix, query_vector):
            check_and_binarize_vectors(query_vector)
        return idx, sc
    finally:
        if owned:
            ix.close()


def rank_batch(vectors, query_vectors, top_k=5, metric='cosine_similarity', timestamps=None, recency_bias=0):
    """Additive: top-k for a (Q, d) batch of independent queries in one pass over the matrix.

    Semantics are exactly "Q calls of hyperDB_ranking_algorithm_sort" (the reference has no batched
    entry: a 2-D query raises or returns garbage there).  Returns (int64 (Q,k), float64 (Q,k))."""
    ix, _, owned = _resolve(vectors)
    try:
        qh = _query_host(query_vectors)
        if qh.ndim == 1:
            qh = qh.reshape(1, -1)
        if ix.has_nan or np.isnan(qh).any():
            raise ValueError(NAN_MESSAGE)
        _validate_metric(metric)
        if ix.n == 0:
            raise ValueError("vectors is empty")
        k = max(0, min(int(top_k), ix.n))
        if k == 0:
            return np.zeros((qh.shape[0], 0), np.int64), np.zeros((qh.shape[0], 0), np.float64)
        had_bias = _apply_recency(ix, timestamps, recency_bias)
        try:
            idx, sc = ix.topk(qh, k, METRIC_IDS[metric])
        finally:
            if had_bias:
                ix.set_bias(None)
        return idx.astype(np.int64), sc.astype(np.float64)
    finally:
        if owned:
            ix.close()


def _single_index(vectors, what):
    """The GpuIndex behind a handle of the rerank entry points; sharded and group handles are not served (ids would need routing)."""
    ix = vectors.index if isinstance(vectors, ResidentVectors) else vectors
    if not isinstance(ix, GpuIndex):
        raise NotImplementedError(f"{what}: needs an index on one device (register_vectors without devices=, or a GpuIndex); "
                                  "sharded and group handles are not served")
    return ix


def rerank_batch(vectors, query_vectors, candidates, top_k=5, metric='cosine_similarity', timestamps=None, recency_bias=0):
    """Additive: the exact top-k of every query among ITS OWN candidate rows -- the second half of a two-stage search, of hybrid
    search (candidates from a keyword index) and of per-query filters.

    ``candidates`` is ``[Q, m]`` row ids (``1 <= m <= 8192``), a host array or an int64 CUDA tensor; ``-1`` is padding, an id
    listed twice counts once, an id outside the index raises IndexError.  Returns ``(int64 (Q, k), float64 (Q, k))`` with
    ``k = min(top_k, m)``, ordered by (score descending, id ascending); where a list holds fewer than k valid rows the tail is
    ``-1`` / ``-inf``.  The scores are those a full ranking gives the same rows; recency is applied as in :func:`rank_batch`.
    Not served: ``storage="bits"`` indexes, hamming and jaccard (NotImplementedError), sharded handles."""
    ix, _, owned = _resolve(vectors)
    try:
        if not isinstance(ix, GpuIndex):
            raise NotImplementedError("rerank_batch: sharded and group handles are not served")
        qh = _query_host(query_vectors)
        if qh.ndim == 1:
            qh = qh.reshape(1, -1)
        if ix.has_nan or np.isnan(qh).any():
            raise ValueError(NAN_MESSAGE)
        _validate_metric(metric)
        m = _native.check_candidates(candidates, qh.shape[0], ix.n, ix.row_base)
        k = max(0, min(int(top_k), m))
        if k == 0:
            return np.zeros((qh.shape[0], 0), np.int64), np.zeros((qh.shape[0], 0), np.float64)
        had_bias = _apply_recency(ix, timestamps, recency_bias)
        try:
            idx, sc = ix.rerank(qh, candidates, k, METRIC_IDS[metric])
        finally:
            if had_bias:
                ix.set_bias(None)
        return idx.astype(np.int64), sc.astype(np.float64)
    finally:
        if owned:
            ix.close()


def rank_two_stage(first, second, query_vectors, top_k=5, oversample=4, metric='cosine_similarity', first_metric=None,
                   first_queries=None):
    """Additive: two-stage search in ONE library call.  The index ``first`` (typically ``storage="bits"``) retrieves
    ``k1 = min(top_k * oversample, 8192, n)`` candidates per query, the index ``second`` over the same rows (int8 or float)
    rescores them exactly with ``metric`` and the best ``min(top_k, k1)`` come back as ``(int64 (Q, k), float64 (Q, k))``.

    ``first_metric`` defaults to ``metric``; ``first_queries`` defaults to ``query_vectors`` -- pass packed ``uint8`` queries for
    a hamming first stage over a bits index.  Both handles are registered indexes on one device with the same rows: ValueError
    when they differ in n, row_base or device, NotImplementedError for sharded or group handles."""
    ix1, ix2 = _single_index(first, "rank_two_stage"), _single_index(second, "rank_two_stage")
    if ix1.n != ix2.n or ix1.row_base != ix2.row_base or ix1.device != ix2.device:
        raise ValueError("rank_two_stage: the two indexes must hold the same rows (n, row_base) on the same device")
    fm = metric if first_metric is None else first_metric
    _validate_metric(metric)
    _validate_metric(fm)
    qh = _query_host(query_vectors)
    if qh.ndim == 1:
        qh = qh.reshape(1, -1)
    q1 = qh if first_queries is None else _query_host(first_queries)
    if q1.ndim == 1:
        q1 = q1.reshape(1, -1)
    if ix1.has_nan or ix2.has_nan or np.isnan(qh).any() or np.isnan(q1).any():
        raise ValueError(NAN_MESSAGE)
    if ix2.n == 0:
        raise ValueError("vectors is empty")
    k1 = max(0, min(int(top_k) * int(oversample), _native.CAND_CAP, ix2.n))
    k = max(0, min(int(top_k), k1))
    if k == 0:
        return np.zeros((qh.shape[0], 0), np.int64), np.zeros((qh.shape[0], 0), np.float64)
    idx, sc = ix2.two_stage(ix1, q1, METRIC_IDS[fm], k1, qh, METRIC_IDS[metric], k)
    return idx.astype(np.int64), sc.astype(np.float64)


def rank_grouped(vectors, query_vectors, groups, top_k=5, metric='cosine_similarity', timestamps=None, recency_bias=0):
    """Additive: one hit per group -- the best row of each group, ``top_k`` distinct groups per query ("group by" / "collapse" of
    a store whose rows are chunks of documents).

    ``groups`` is one integer id per row (numpy or torch).  The rows of a query are ordered as :func:`rank_batch` orders them
    (score descending, row ascending, recency applied); a group is represented by its first row in that order, and the first
    ``k = min(top_k, n)`` representatives come back as ``(int64 (Q, k) rows, float64 (Q, k) scores, int64 (Q, k) group ids)``;
    where fewer than k groups exist the tail is ``-1`` / ``-inf`` / ``-1``.  ``vectors`` is a registered handle on one device or a
    raw matrix registered for the call; sharded and group handles raise NotImplementedError (a group can span shards), and so do
    hamming and jaccard and ``top_k`` beyond 2048."""
    if isinstance(vectors, ResidentVectors) and not isinstance(vectors.index, GpuIndex) or isinstance(vectors, GpuGroup):
        raise NotImplementedError("rank_grouped: needs an index on one device; a group of rows can span the shards of a sharded handle")
    ix, _, owned = _resolve(vectors)
    try:
        if not isinstance(ix, GpuIndex):
            raise NotImplementedError("rank_grouped: needs an index on one device; a group of rows can span the shards of a sharded handle")
        qh = _query_host(query_vectors)
        if qh.ndim == 1:
            qh = qh.reshape(1, -1)
        if ix.has_nan or np.isnan(qh).any():
            raise ValueError(NAN_MESSAGE)
        _validate_metric(metric)
        if ix.n == 0:
            raise ValueError("vectors is empty")
        k = max(0, min(int(top_k), ix.n))
        if k == 0:
            z = np.zeros((qh.shape[0], 0), np.int64)
            return z, np.zeros((qh.shape[0], 0), np.float64), z.copy()
        ix.set_groups(groups)
        had_bias = _apply_recency(ix, timestamps, recency_bias)
        try:
            idx, sc = ix.topk_grouped(qh, k, METRIC_IDS[metric])
            gh = ix._groups.cpu().numpy().astype(np.int64)
        finally:
            ix.set_groups(None)
            if had_bias:
                ix.set_bias(None)
        idx = idx.astype(np.int64)
        gid = np.where(idx >= 0, gh[np.clip(idx - ix.row_base, 0, ix.n - 1)], -1)
        return idx, sc.astype(np.float64), gid
    finally:
        if owned:
            ix.close()


def rank_maxsim(vectors, query_sets, groups=None, top_k=5, metric='cosine_similarity'):
    """Additive: multi-vector queries -- groups ranked by the sum over a set's vectors of each vector's best row in the group (late
    interaction over token / patch vectors; fusion of several paraphrases of one question over the chunks of documents).

    ``query_sets`` is a ``(T, d)`` array (one set), an ``(S, T, d)`` array or a list of ``(T_i, d)`` arrays; ``groups`` one integer
    id per row, ``None`` = every row its own group (the rows ranked by their summed scores).  Returns ``(int64 (S, k) group ids,
    float64 (S, k) scores)``, ``k = min(top_k, n_groups)``, score descending, group id ascending; where fewer than k groups have an
    eligible row for every vector the tail is ``-1`` / ``-inf``.  A bias set on the handle enters every term, so T times in all.
    ``vectors`` is a registered handle on one device or a raw matrix registered for the call; sharded and group handles raise
    NotImplementedError, and so do hamming and jaccard and ``top_k`` beyond 2048."""
    if isinstance(vectors, ResidentVectors) and not isinstance(vectors.index, GpuIndex) or isinstance(vectors, GpuGroup):
        raise NotImplementedError("rank_maxsim: needs an index on one device; a group of rows can span the shards of a sharded handle")
    ix, _, owned = _resolve(vectors)
    try:
        if not isinstance(ix, GpuIndex):
            raise NotImplementedError("rank_maxsim: needs an index on one device; a group of rows can span the shards of a sharded handle")
        flat, off = pack_query_sets(query_sets, ix.d)
        if ix.has_nan or np.isnan(flat).any():
            raise ValueError(NAN_MESSAGE)
        _validate_metric(metric)
        if ix.n == 0:
            raise ValueError("vectors is empty")
        ns = int(off.size) - 1
        ids = np.arange(ix.n, dtype=np.int32) if groups is None else groups
        ix.set_groups(ids)
        try:
            k = max(0, min(int(top_k), ix.n_groups))
            if k == 0:
                return np.zeros((ns, 0), np.int64), np.zeros((ns, 0), np.float64)
            gid, sc = ix.maxsim(flat, off, k, METRIC_IDS[metric])
        finally:
            ix.set_groups(None)
        return gid.astype(np.int64), sc.astype(np.float64)
    finally:
        if owned:
            ix.close()


def rank_mmr(vectors, query_vectors, top_k=5, fetch_k=None, lambda_mult=0.5, metric='cosine_similarity', pair_metric=None, timestamps=None,
             recency_bias=0):
    """Additive: a diverse top-k -- maximal marginal relevance.  The ``fetch_k`` best rows of every query are fetched as
    :func:`rank_batch` ranks them (recency applied), and ``top_k`` of them are picked one after the other: the first by relevance,
    each later one by ``lambda_mult * relevance - (1 - lambda_mult) * (largest similarity to a row already picked)``.  A near copy
    of a hit already chosen pays for it; ``lambda_mult=1`` is :func:`rank_batch`, ``0`` is relevance first and then the least
    similar.

    Returns ``(int64 (Q, k) rows, float64 (Q, k) relevances)`` IN PICK ORDER, ``k = min(top_k, n)``.  ``fetch_k=None`` means
    ``min(n, 2048, 4 * top_k)`` (the factor of ``oversample``, by analogy and not measured); at most 2048.  ``pair_metric`` -- dot,
    cosine or euclidean between stored rows -- defaults to ``metric`` where that is one of the three, to cosine otherwise; another
    one raises NotImplementedError, and so does a ``storage="bits"`` handle.  ``vectors`` is a registered handle on one device or a
    raw matrix registered for the call; sharded and group handles raise NotImplementedError: the candidates' rows live on
    different shards."""
    one_device = "rank_mmr: needs an index on one device; the candidates of a query live on different shards of a sharded handle"
    if isinstance(vectors, ResidentVectors) and not isinstance(vectors.index, GpuIndex) or isinstance(vectors, GpuGroup):
        raise NotImplementedError(one_device)
    ix, _, owned = _resolve(vectors)
    try:
        if not isinstance(ix, GpuIndex):
            raise NotImplementedError(one_device)
        qh = _query_host(query_vectors)
        if qh.ndim == 1:
            qh = qh.reshape(1, -1)
        _validate_metric(metric)
        pm = pair_metric if pair_metric is not None else (metric if metric in _native.PAIR_METRICS else "cosine_similarity")
        _validate_metric(pm)
        if pm not in _native.PAIR_METRICS:
            raise NotImplementedError(f"rank_mmr: pair_metric {pm!r} is not built (dot, cosine and euclidean are)")
        if ix.dtype == _native.HDB_B1:
            raise NotImplementedError("rank_mmr: a storage='bits' index is a first stage; pair similarity of packed bits is not built")
        if not 0.0 <= float(lambda_mult) <= 1.0:
            raise ValueError(f"rank_mmr: lambda_mult must be in [0, 1], got {lambda_mult!r}")
        if ix.has_nan or np.isnan(qh).any():
            raise ValueError(NAN_MESSAGE)
        if ix.n == 0:
            raise ValueError("vectors is empty")
        k = max(0, min(int(top_k), ix.n))
        if k == 0:
            return np.zeros((qh.shape[0], 0), np.int64), np.zeros((qh.shape[0], 0), np.float64)
        m = min(ix.n, _native.HDB_MAX_K, 4 * k) if fetch_k is None else min(int(fetch_k), ix.n)
        m = max(m, k)
        had_bias = _apply_recency(ix, timestamps, recency_bias)
        try:
            idx, sc = ix.mmr(qh, m, k, METRIC_IDS[metric], float(lambda_mult), METRIC_IDS[pm])
        finally:
            if had_bias:
                ix.set_bias(None)
        return idx.astype(np.int64), sc.astype(np.float64)
    finally:
        if owned:
            ix.close()
