"""ctypes binding of libhyperdb_hip.so (include/hyperdb_hip.h) + the resident-matrix handle.

This is the only place where Python touches the C ABI.  PyTorch-ROCm is used for device memory,
streams and H2D/D2H copies only; every score and every top-k comes out of the hand-written HIP
kernels.  There is no CPU fallback: if the library is missing, importing this module raises.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict

import numpy as np
import torch  # must be imported before the .so so that ONE libamdhip64 (torch's) serves both

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HYPERDB_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libhyperdb_hip.so")

HDB_F16, HDB_F32, HDB_F64, HDB_BF16 = 0, 1, 2, 3
HDB_F8E4M3 = 5                          # OCP float8 e4m3 (torch.float8_e4m3fn); 4 is unassigned and refused by the library
HDB_I8 = 7                              # signed 8-bit integers (np.int8 / torch.int8), on request: storage="int8"; 6 is unassigned
HDB_B1 = 10                             # packed bits, one bit per element, on request: storage="bits"; 8 and 9 are unassigned
METRIC_IDS = {
    "dot_product": 0,
    "cosine_similarity": 1,
    "euclidean_metric": 2,
    "hamming_distance": 3,
    "manhattan_distance": 4,
    "jaccard_similarity": 5,
    "pearson_correlation": 6,
}
EUCLIDEAN_DIST = 7
Q_UNDERFLOW, Q_OVERFLOW, Q_NAN = 1, 2, 4
Q_BADROW = 8                            # hdb_rerank: a candidate id outside the index (skipped, never read)
Q_GROUPS_SHORT = 16                     # hdb_collapse_groups: fewer than k groups in a list that was not exhaustive
CAND_CAP = 8192                         # longest candidate list of a rerank call (HDB_CAND_CAP)
HDB_QUANT_NONE, HDB_QUANT_I8 = 0, 1
QUANT_MODES = {None: HDB_QUANT_NONE, "int8": HDB_QUANT_I8}
HDB_MAX_K = 2048
PAIR_METRICS = ("dot_product", "cosine_similarity", "euclidean_metric")      # what two stored rows can be compared by (hdb_mmr)
MERGE_DEVICE_CAP = 8192      # hdb_merge_topk / hdb_merge_topk_packed rank parts*k entries per query in LDS; beyond: hdb_merge_topk_host

NAN_MESSAGE = "Vectors and query_vector should not contain NaN values."   # reference ranking_algorithm.py:151

EXPORTS = (
    "hdb_version", "hdb_last_error", "hdb_index_create", "hdb_index_update", "hdb_index_rebase", "hdb_index_extend",
    "hdb_index_gather", "hdb_index_set_row_base", "hdb_index_destroy",
    "hdb_group_create", "hdb_group_topk_host", "hdb_group_destroy",
    "hdb_index_has_nan", "hdb_index_set_bias", "hdb_index_set_row_mask", "hdb_scores", "hdb_topk",
    "hdb_topk_exact", "hdb_merge_topk", "hdb_set_option", "hdb_get_stat", "hdb_recency_bias", "hdb_recency_bias_twice",
    "hdb_packed_bytes", "hdb_merge_topk_packed", "hdb_merge_topk_host", "hdb_host_exchange_merge", "hdb_topk_host",
    "hdb_index_quantize", "hdb_debug_quant_bounds", "hdb_index_set_row_subset",
    "hdb_rerank", "hdb_rerank_host", "hdb_two_stage_host",
    "hdb_index_set_groups", "hdb_topk_grouped_host", "hdb_collapse_groups",
    "hdb_maxsim_host",
    "hdb_mmr", "hdb_mmr_host",
)


class HyperDBNativeError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the MI355X HIP extension has not been built. "
            "Run `python __graft_entry__.py` (or local-hyperdb_amd/csrc/build.sh). "
            "There is deliberately no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, cp = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_char_p
    lib.hdb_version.restype = ctypes.c_int
    lib.hdb_last_error.restype = cp
    lib.hdb_index_create.argtypes = [ctypes.POINTER(vp), vp, i64, i32, ctypes.c_int, ctypes.c_int, i64, vp]
    lib.hdb_index_update.argtypes = [vp, vp, i64, vp]
    lib.hdb_index_rebase.argtypes = [vp, vp]
    lib.hdb_index_extend.argtypes = [vp, i64, vp]
    lib.hdb_index_gather.argtypes = [vp, vp, i64, vp, vp]
    lib.hdb_index_set_row_base.argtypes = [vp, i64]
    lib.hdb_index_quantize.argtypes = [vp, ctypes.c_int, vp]
    lib.hdb_debug_quant_bounds.argtypes = [vp, vp, ctypes.c_int, vp, vp, vp]
    lib.hdb_group_create.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(vp), i32]
    lib.hdb_group_topk_host.argtypes = [vp, vp, i32, i32, ctypes.c_int, vp]
    lib.hdb_group_destroy.argtypes = [vp]
    lib.hdb_group_destroy.restype = None
    lib.hdb_index_destroy.argtypes = [vp]
    lib.hdb_index_destroy.restype = None
    lib.hdb_index_has_nan.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    lib.hdb_index_set_bias.argtypes = [vp, vp]
    lib.hdb_index_set_row_mask.argtypes = [vp, vp]
    lib.hdb_index_set_row_subset.argtypes = [vp, vp, vp, i64]
    lib.hdb_scores.argtypes = [vp, vp, ctypes.c_int, vp, vp]
    lib.hdb_topk.argtypes = [vp, vp, i32, i32, ctypes.c_int, vp, vp, vp, vp]
    lib.hdb_topk_exact.argtypes = [vp, vp, i32, i32, ctypes.c_int, vp, vp, vp, vp]
    lib.hdb_merge_topk.argtypes = [vp, vp, i32, i32, i32, vp, vp, ctypes.c_int, vp]
    lib.hdb_set_option.argtypes = [vp, cp, i64]
    lib.hdb_get_stat.argtypes = [vp, cp, ctypes.POINTER(i64)]
    lib.hdb_recency_bias.argtypes = [vp, i64, ctypes.c_double, ctypes.c_double, vp, ctypes.c_int, vp]
    lib.hdb_recency_bias_twice.argtypes = [vp, vp, i64, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, ctypes.c_int, vp]
    lib.hdb_topk_host.argtypes = [vp, vp, i32, i32, ctypes.c_int, vp, vp]
    lib.hdb_packed_bytes.argtypes = [i32, i32]
    lib.hdb_rerank.argtypes = [vp, vp, i32, vp, i32, i32, ctypes.c_int, vp, vp, vp, vp]
    lib.hdb_rerank_host.argtypes = [vp, vp, i32, vp, i32, i32, ctypes.c_int, vp, vp]
    lib.hdb_two_stage_host.argtypes = [vp, vp, ctypes.c_int, i32, vp, vp, ctypes.c_int, i32, i32, vp, vp]
    lib.hdb_index_set_groups.argtypes = [vp, vp, i64]
    lib.hdb_topk_grouped_host.argtypes = [vp, vp, i32, i32, ctypes.c_int, vp, vp]
    lib.hdb_collapse_groups.argtypes = [vp, vp, i32, i32, i32, vp, i64, i64, i64, vp, vp, vp, ctypes.c_int, vp]
    lib.hdb_maxsim_host.argtypes = [vp, vp, vp, i32, i32, ctypes.c_int, vp, vp]
    lib.hdb_mmr.argtypes = [vp, vp, vp, i32, i32, i32, ctypes.c_double, ctypes.c_int, vp, vp, vp, vp]
    lib.hdb_mmr_host.argtypes = [vp, vp, i32, i32, i32, ctypes.c_int, ctypes.c_double, ctypes.c_int, vp, vp]
    lib.hdb_merge_topk_packed.argtypes = [vp, i32, i32, i32, vp, vp, vp, ctypes.c_int, vp]
    lib.hdb_merge_topk_host.argtypes = [vp, i32, i32, i32, vp]
    lib.hdb_host_exchange_merge.argtypes = [vp, i64, i32, i32, ctypes.c_uint64, vp, i32, i32, vp, ctypes.c_double]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("hdb_last_error", "hdb_index_destroy", "hdb_group_destroy", "hdb_packed_bytes"):
            fn.restype = ctypes.c_int
    lib.hdb_packed_bytes.restype = i64
    return lib


_lib = _load()


def lib():
    return _lib


def _check(rc, what):
    if rc == 0:
        return
    msg = _lib.hdb_last_error().decode("utf-8", "replace")
    if rc == -1:
        raise ValueError(f"{what}: {msg}")
    if rc == -3:
        raise NotImplementedError(f"{what}: {msg}")
    raise HyperDBNativeError(f"{what}: {msg} (status {rc})")


def require_gpu():
    if not torch.cuda.is_available():
        raise HyperDBNativeError(
            "no MI355X visible: the HyperDB ranking path runs only on the GPU (no CPU fallback).")


_NP2HDB = {np.dtype(np.float16): HDB_F16, np.dtype(np.float32): HDB_F32, np.dtype(np.float64): HDB_F64}
# (numpy has no bfloat16: a bf16 matrix arrives as a torch tensor and leaves as its exact float32 widening)
# (... nor float8: an e4m3 matrix arrives as a torch.float8_e4m3fn tensor, one byte per element, and leaves the same way)
_F8 = torch.float8_e4m3fn
_TORCH2HDB = {torch.float16: HDB_F16, torch.float32: HDB_F32, torch.float64: HDB_F64, torch.bfloat16: HDB_BF16, _F8: HDB_F8E4M3}
F8_MAX = 448.0                          # largest finite e4m3 magnitude
# what a STORED tensor's dtype is to the library.  torch.int8 is in here and not in _TORCH2HDB: without storage="int8" an int8
# tensor is widened to float64 like every other integer input (to_device_matrix), with it the bytes are the matrix
_STORED2HDB = dict(_TORCH2HDB)
_STORED2HDB[torch.int8] = HDB_I8
# ... and torch.uint8: the packed rows of a bits index (storage="bits"); without the keyword a uint8 input is widened to float64
_STORED2HDB[torch.uint8] = HDB_B1
STORAGE_MODES = (None, "int8", "bits")
BITORDERS = ("big", "little")
BITS_SINGLE_INDEX = ("storage='bits' is built for a single index on one device only (GpuIndex, register_vectors without "
                     "devices=): no GpuGroup, no sharded index, no HyperDB facade")


def storage_mode(storage):
    """A ``storage=`` argument: None (the input's own dtype policy), "int8" or "bits"; anything else raises ValueError."""
    if storage is not None and not isinstance(storage, str) or storage not in STORAGE_MODES:
        raise ValueError(f"storage must be None, 'int8' or 'bits', got {storage!r}")
    return storage


def bit_order(bitorder):
    """A ``bitorder=`` argument: "big" (np.packbits' default, what embedding exports use) or "little"."""
    if bitorder not in BITORDERS:
        raise ValueError(f"bitorder must be 'big' or 'little', got {bitorder!r}")
    return bitorder


def pack_bits(X, bitorder="big"):
    """Any numeric or bool ``[n, d]`` -> packed uint8 ``[n, d/8]`` by ``X > 0``, the reference's own binarisation
    (check_and_binarize_vectors): what storage="bits" takes.  d must be a multiple of 32 (ValueError otherwise)."""
    bit_order(bitorder)
    if isinstance(X, torch.Tensor):
        t = X.detach().cpu()
        if t.dtype in (torch.bfloat16, torch.float16, _F8):
            t = t.to(torch.float32)
        X = t.numpy()
    a = np.asarray(X)
    if a.dtype != np.bool_ and (not np.issubdtype(a.dtype, np.number) or np.issubdtype(a.dtype, np.complexfloating)):
        raise ValueError("pack_bits: vectors must be numeric or bool")
    if a.ndim != 2:
        raise ValueError(f"pack_bits: vectors must be 2-D (N x d), got shape {tuple(a.shape)}")
    if a.shape[1] == 0 or a.shape[1] % 32 != 0:
        raise ValueError(f"pack_bits: d must be a multiple of 32, got {a.shape[1]}")
    bits = a if a.dtype == np.bool_ else a > 0
    return np.packbits(bits, axis=1, bitorder=bitorder)


def reverse_bits8(t):
    """Every byte of a torch.uint8 tensor with its bits reversed (big <-> little bit order), on the tensor's own device: three
    swap steps of byte-wise masks and shifts, no table."""
    t = ((t & 0xF0) >> 4) | ((t & 0x0F) << 4)
    t = ((t & 0xCC) >> 2) | ((t & 0x33) << 2)
    return ((t & 0xAA) >> 1) | ((t & 0x55) << 1)


_BITS_POLICY = ("storage='bits' takes packed rows (2-D uint8, [n, d/8]) or unpacked bits (2-D bool, [n, d]) with d a multiple of "
                "32 and binarises nothing itself: pack other data with hyperdb._native.pack_bits(X) (x > 0) first")


def _bits_check(data):
    """The input policy of storage="bits" -> ("bool" | "packed", the 2-D tensor or array); ValueError naming pack_bits otherwise."""
    if isinstance(data, torch.Tensor):
        x, dt, shape = data.detach(), data.dtype, tuple(data.shape)
        kind = "bool" if dt == torch.bool else "packed" if dt == torch.uint8 else None
    else:
        x = data if isinstance(data, np.ndarray) else np.asarray(data)
        dt, shape = x.dtype, tuple(x.shape)
        kind = "bool" if dt == np.bool_ else "packed" if dt == np.uint8 else None
    if kind is None or len(shape) != 2:
        raise ValueError(f"{_BITS_POLICY}; got {dt} data of shape {shape}")
    bits = shape[1] * (8 if kind == "packed" else 1)
    if bits == 0 or bits % 32 != 0:
        raise ValueError(f"{_BITS_POLICY}; got {bits} bits per row")
    return kind, x


def to_bits(data, device, bitorder="big"):
    """The input of a bits index -> contiguous torch.uint8 ``[n, d/8]`` on `device` in the LITTLE bit order the library reads
    (element e of a row = bit e & 7 of byte e >> 3).  Takes only a 2-D uint8 array / tensor of packed rows in `bitorder` (host or
    device) and a 2-D bool array / tensor of unpacked bits (packed on the host); anything else raises ValueError naming pack_bits.
    Big-order bytes are bit-reversed once, on `device`."""
    bit_order(bitorder)
    kind, x = _bits_check(data)
    if kind == "bool":
        h = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        return torch.from_numpy(pack_bits(h, "little")).to(device).contiguous()
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.to(device)
    t = reverse_bits8(t) if bitorder == "big" else t
    return t.contiguous()


def unpack_bits_host(packed, bitorder):
    """Packed uint8 ``[..., d/8]`` (numpy) -> the float32 0/1 array ``[..., d]``."""
    return np.unpackbits(np.ascontiguousarray(packed), axis=-1, bitorder=bitorder).astype(np.float32)


def to_i8(data):
    """Numeric data -> torch.int8 tensor for an int8 index (storage="int8"), on the host.  An int8 tensor or array goes in as it
    is (``to_i8(t) is t`` for a torch.int8 tensor, wherever it lives).  Anything else numeric is accepted only if every element is
    an integer in [-128, 127]; otherwise ValueError names the first offending value -- no rounding, no scaling, no saturation."""
    if isinstance(data, torch.Tensor):
        if data.dtype == torch.int8:
            return data
        t = data.detach().cpu()
        if t.dtype in (torch.bfloat16, torch.float16, _F8):
            t = t.to(torch.float32)                     # (exact; numpy has no bfloat16 / float8)
        a = t.numpy()
    else:
        a = np.asarray(data)
    if a.dtype == np.int8:
        return torch.from_numpy(np.ascontiguousarray(a))
    if a.dtype == np.bool_:
        a = a.astype(np.int8)
    elif not np.issubdtype(a.dtype, np.number) or np.issubdtype(a.dtype, np.complexfloating):
        raise ValueError("vectors must be numeric")
    else:
        ok = (a >= -128) & (a <= 127)                   # (NaN compares false; inf is out of range)
        if a.dtype.kind == "f":
            with np.errstate(invalid="ignore"):
                ok &= a == np.floor(a)
        if not ok.all():
            bad = a[~ok].reshape(-1)[0]
            raise ValueError(f"storage='int8' takes integers in [-128, 127] and stores them as they are; got {bad!r} "
                             "(quantise float embeddings before handing them over)")
        a = a.astype(np.int8)
    return torch.from_numpy(np.ascontiguousarray(a))


def _as_bytes(t):
    """A float8 tensor as its uint8 view (same storage): copies, indexing and allocation of one-byte rows go through uint8, for
    which every torch build has device kernels; any other tensor as it is."""
    return t.view(torch.uint8) if t.dtype == _F8 else t


def to_f8(data):
    """Float data -> host torch.float8_e4m3fn tensor with torch's own conversion: round to nearest even, magnitudes up to 464
    round to 448 and anything beyond becomes NaN (torch does not saturate).  Done on the host, before upload."""
    if isinstance(data, torch.Tensor):
        if data.dtype == _F8:
            return data                                 # already float8, wherever it lives
        t = data.detach().cpu()
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(data)))
    return t.to(torch.float32).to(_F8)


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # the current stream's handle without building a Stream object (0.3 vs 1.5 us)


def _stream_int(device):
    if _raw_stream is not None:
        return _raw_stream(device.index or 0)
    return torch.cuda.current_stream(device).cuda_stream


def _stream_ptr(device):
    return ctypes.c_void_p(_stream_int(device))


def to_device_matrix(vectors, device, storage=None):
    """numpy / list / torch -> C-contiguous 2-D torch tensor on `device` in a supported dtype.

    storage="int8": the input is converted with to_i8 (int8 stays, integers in [-128, 127] of any numeric dtype are taken,
    anything else raises ValueError) and travels as torch.int8.  Without it nothing below changes: integer inputs, torch.int8
    included, are widened to float64.

    Dtype policy mirrors HyperDB.fp_precision (hyperdb.py:65-66): float16/32/64 stay as they are (and so does a
    torch.bfloat16 tensor: 2 bytes per element on the device; and a torch.float8_e4m3fn tensor: 1 byte), anything else numeric (ints, bools) is widened to float64 like numpy would promote it."""
    if storage_mode(storage) == "int8":
        return to_i8(vectors).to(device).contiguous()
    if isinstance(vectors, torch.Tensor):
        t = vectors
        if t.dtype not in _TORCH2HDB:
            t = t.to(torch.float64)
        if t.dtype == _F8:                  # the bytes travel as uint8
            return t.contiguous().view(torch.uint8).to(device).view(_F8)
        return t.to(device).contiguous()
    arr = np.asarray(vectors)
    if arr.dtype not in _NP2HDB:
        if not (np.issubdtype(arr.dtype, np.number) or arr.dtype == np.bool_):
            raise ValueError("vectors must be numeric")
        arr = arr.astype(np.float64)
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr).to(device, non_blocking=False)


class GpuIndex:
    """A resident N x d matrix on one MI355X plus its per-row caches (hdb_index handle).

    Replaces the per-query work of reference ranking_algorithm.py:150 (NaN scan), :153 (copy) and
    :37 (re-normalising every row): those happen once here, at registration.
    """

    def __init__(self, vectors, device=None, row_base=0, storage=None, bitorder="big"):
        storage_mode(storage)
        self.bitorder = bit_order(bitorder)    # storage="bits": the order of the caller's packed bytes (the device holds "little")
        if storage == "bits":
            _bits_check(vectors)               # (the input policy: ValueError before a GPU is asked for)
        require_gpu()
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = torch.device(device)
        t = to_bits(vectors, self.device, bitorder) if storage == "bits" else to_device_matrix(vectors, self.device, storage)
        if t.dim() != 2:
            # reference: non-2-D vectors make the metric functions raise (tests/test_ranking_algorithm.py:107-114)
            raise ValueError(f"vectors must be 2-D (N x d), got shape {tuple(t.shape)}")
        self.V = t
        self.n, self.d = int(t.shape[0]), int(t.shape[1])
        if storage == "bits":
            self.d *= 8                        # d counts bits; V is the uint8 tensor [n, d / 8]
        if self.d == 0:
            raise ValueError("vectors must have d > 0")
        self._cols = int(t.shape[1])           # columns of the stored tensor: d, or d / 8 bytes of a bits index
        self.dtype = _STORED2HDB[t.dtype]
        self.storage = storage                 # "int8": append / update convert with to_i8; "bits": with to_bits
        self.row_base = int(row_base)
        self._h = ctypes.c_void_p()
        self._bias = None
        self._mask = None
        self._rows = None                      # the row list set beside the mask (set_row_subset)
        self._rows_ok = OrderedDict()          # id(device list) -> the list: validated once, kept alive so the id stays its own
        self._groups = None                    # the group id per row (set_groups), int32 on the device
        self.n_groups = 0
        self._groups_ok = OrderedDict()        # id(device ids) -> (the ids, their maximum + 1): validated once, as _rows_ok
        self._nan = None
        self._buf = None
        self.quant = HDB_QUANT_NONE             # int8 shadow (quantize)
        self._qstage = OrderedDict()           # (nq, dtype) -> (pinned host tensor, its numpy view, device tensor or None, address the kernels read)
        self._host_records = OrderedDict()     # (nq, k) -> pinned record + views, owned by THIS index (small LRU)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_index_create(ctypes.byref(self._h), ctypes.c_void_p(t.data_ptr()), self.n, self.d,
                                         self.dtype, self.device.index or 0, self.row_base,
                                         _stream_ptr(self.device)), "hdb_index_create")

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.hdb_index_destroy(self._h)
            self._h = ctypes.c_void_p()
        if getattr(self, "_host_records", None):
            self._host_records.clear()                 # releases the pinned host memory
        if getattr(self, "_qstage", None):
            self._qstage.clear()
        self._buf = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append(self, rows):
        """Append rows behind the stored ones (HyperDB.add): amortised O(new rows).  The device allocation grows
        by doubling; the library re-points (hdb_index_rebase) and extends its row caches (hdb_index_extend)."""
        if self.dtype == HDB_F8E4M3:
            rows = to_f8(rows)                              # float data into a float8 index: torch's conversion, on the host
        if self.dtype == HDB_B1:
            t = to_bits(rows, self.device, self.bitorder)          # (packed uint8 or bool rows only -- ValueError before anything is stored)
        else:
            t = to_device_matrix(rows, self.device, self.storage)      # (an int8 index: to_i8 -- ValueError before anything is stored)
        if t.dim() == 1:
            t = t.reshape(1, -1)
        if t.dim() != 2 or int(t.shape[1]) != self._cols:
            raise ValueError(f"append: rows must have {self.d} columns")
        if t.dtype != self.V.dtype:
            t = t.to(self.V.dtype)
        m = int(t.shape[0])
        if m == 0:
            return
        buf = self._buf
        if buf is None or buf.data_ptr() != self.V.data_ptr():
            buf = self.V                                    # first append: the registered tensor is the buffer
        cap = int(buf.shape[0])
        if self.n + m > cap:
            new_cap = max(self.n + m, 2 * cap, 1024)
            nbuf = torch.empty((new_cap, self._cols), dtype=_as_bytes(self.V).dtype, device=self.device).view(self.V.dtype)
            _as_bytes(nbuf)[:self.n].copy_(_as_bytes(self.V))
            buf = nbuf
            _check(_lib.hdb_index_rebase(self._h, ctypes.c_void_p(buf.data_ptr())), "hdb_index_rebase")
        _as_bytes(buf)[self.n:self.n + m].copy_(_as_bytes(t))
        self._buf = buf
        self.n += m
        self.V = buf[:self.n]
        self._bias = self._mask = None
        self._forget_rows()
        self._nan = None
        _check(_lib.hdb_index_extend(self._h, self.n, _stream_ptr(self.device)), "hdb_index_extend")

    def update(self, vectors):
        """Point the handle at a new matrix (after add/remove) and rebuild the row caches."""
        if self.dtype == HDB_F8E4M3:
            vectors = to_f8(vectors)                        # ... into a float8 index: torch's conversion, on the host, as append does
        if self.dtype == HDB_B1:
            t = to_bits(vectors, self.device, self.bitorder)       # (a bits index: packed uint8 or bool rows, as append does)
        else:
            t = to_device_matrix(vectors, self.device, self.storage)   # (an int8 index: to_i8, as append does)
        if self.dtype == HDB_BF16 and t.dtype != torch.bfloat16:
            t = t.to(torch.bfloat16)                        # float data into a bf16 index: round to nearest even, as append does
        if t.dim() != 2 or int(t.shape[1]) != self._cols or _STORED2HDB.get(t.dtype) != self.dtype:
            raise ValueError("update: matrix must keep d and dtype")
        self.V, self.n = t, int(t.shape[0])
        self._bias = self._mask = self._nan = None
        self._forget_rows()
        self._buf = None                                    # the old capacity buffer is released with the old matrix
        _check(_lib.hdb_index_update(self._h, ctypes.c_void_p(t.data_ptr()), self.n, _stream_ptr(self.device)),
               "hdb_index_update")

    def quantize(self, mode="int8"):
        """Build (``"int8"``) or drop (``None``) the int8 shadow of the matrix (hdb_index_quantize): 1-4-query dot / cosine /
        euclidean calls with k <= 128 then stream one byte per element and rescore the surviving rows exactly -- the same
        indices and float32 scores as without it.  The shadow follows append / update / compact; it costs N x (round_up(d, 16)
        + 12) bytes of device memory.  A large fp16 index also builds a shadow for itself on its first 1-4-query dot / cosine
        call (option ``auto_quant``; that flavour returns the matrix cores' bits, i.e. exactly what the call returned before);
        ``quantize(None)`` drops either kind and switches the automatic build off for this handle, ``quantize("int8")`` keeps
        the explicit meaning.

        bfloat16: opt-in.  ``quantize("int8")`` raises NotImplementedError on a bf16 index unless ``set_option("bf16_quant", 1)``
        came first; with it the shadow is built as for fp16 / fp32 (explicit only, never automatic) and the 1-4-query calls it
        serves return the bits of the VALU scan -- the path a bf16 index takes for such calls by default.  ``register_vectors``
        and ``HyperDB`` set the option themselves when they are given ``quantize="int8"``.  float8, int8 (``storage="int8"``: one
        byte per element already) and float64 raise."""
        mode = quant_mode(mode)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_index_quantize(self._h, mode, _stream_ptr(self.device)), "hdb_index_quantize")
        self.quant = mode

    def quant_bounds(self, q, metric_id):
        """Test helper (hdb_debug_quant_bounds): per row, the int8 pass's upper bound and the 5-bit plane's, for one float32 query
        -> two float32 numpy arrays of n entries.  The index needs a shadow with its plane."""
        qd = torch.from_numpy(np.ascontiguousarray(np.asarray(q, dtype=np.float32).reshape(-1))).to(self.device)
        if qd.numel() != self.d:
            raise ValueError(f"query must have {self.d} entries")
        hi = torch.empty(self.n, dtype=torch.float32, device=self.device)
        hi5 = torch.empty(self.n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_debug_quant_bounds(self._h, ctypes.c_void_p(qd.data_ptr()), int(metric_id), ctypes.c_void_p(hi.data_ptr()),
                                               ctypes.c_void_p(hi5.data_ptr()), _stream_ptr(self.device)), "hdb_debug_quant_bounds")
        return hi.cpu().numpy(), hi5.cpu().numpy()

    def set_row_base(self, row_base):
        self.row_base = int(row_base)
        _check(_lib.hdb_index_set_row_base(self._h, self.row_base), "hdb_index_set_row_base")

    def host_matrix(self):
        """The stored rows as a host array (one D2H copy; the resident copy stays the only one kept).  A bfloat16 index returns
        the exact float32 widening (numpy has no bfloat16), and so do a float8 index (widened on the host) and an int8 index."""
        if self.dtype == HDB_B1:
            return unpack_bits_host(self.V.cpu().numpy(), "little")
        if self.V.dtype == torch.int8:
            return self.V.cpu().numpy().astype(np.float32)
        if self.V.dtype == torch.bfloat16:
            return self.V.float().cpu().numpy()
        if self.V.dtype == _F8:
            return self.V.view(torch.uint8).cpu().view(_F8).float().numpy()
        return self.V.cpu().numpy()

    def host_bits(self):
        """A bits index (storage="bits"): the stored rows as packed uint8 ``[n, d/8]`` in the index's ``bitorder`` -- what went in."""
        if self.dtype != HDB_B1:
            raise ValueError("host_bits: only a storage='bits' index holds packed rows")
        v = reverse_bits8(self.V) if self.bitorder == "big" else self.V
        return v.cpu().numpy()

    def _bits_query(self, q):
        """A bits index: a uint8 query of d/8 bytes (or [nq, d/8]) is packed in the index's bitorder -> its 0/1 float32 form (binary
        query against binary rows); anything else is a query of d elements and passes through."""
        if isinstance(q, torch.Tensor):
            if q.dtype == torch.uint8 and q.dim() in (1, 2) and int(q.shape[-1]) == self._cols:
                sh = torch.arange(7, -1, -1, device=q.device) if self.bitorder == "big" else torch.arange(8, device=q.device)
                return ((q.unsqueeze(-1).to(torch.int32) >> sh.to(torch.int32)) & 1).reshape(*q.shape[:-1], self.d).to(torch.float32)
            return q
        a = q if isinstance(q, np.ndarray) else np.asarray(q)
        if a.dtype == np.uint8 and a.ndim in (1, 2) and a.shape[-1] == self._cols:
            return unpack_bits_host(a, self.bitorder)
        return q

    def compact(self, keep_rows):
        """Keep only the rows `keep_rows` (ascending local row ids): device-side gather into a fresh allocation, the
        row caches travel with their rows (hdb_index_gather) -- the matrix part of HyperDB.remove_document
        (hyperdb.py:691-766) without a host round trip or a cache rebuild."""
        rows = torch.from_numpy(np.ascontiguousarray(np.asarray(keep_rows, dtype=np.int64))).to(self.device)
        m = int(rows.numel())
        out = torch.empty((max(m, 1), self._cols), dtype=_as_bytes(self.V).dtype, device=self.device).view(self.V.dtype)
        _check(_lib.hdb_index_gather(self._h, ctypes.c_void_p(rows.data_ptr()), m, ctypes.c_void_p(out.data_ptr()),
                                     _stream_ptr(self.device)), "hdb_index_gather")
        self._buf = out
        self.V, self.n = out[:m], m
        self._bias = self._mask = self._nan = None
        self._forget_rows()

    @property
    def has_nan(self):
        if self._nan is None:
            flag = ctypes.c_int(0)
            _check(_lib.hdb_index_has_nan(self._h, ctypes.byref(flag)), "hdb_index_has_nan")
            self._nan = bool(flag.value)
        return self._nan

    # -- per-row additive term / row subset ----------------------------------------------------
    def set_bias(self, bias):
        """bias: None, or N floats (numpy / torch) added to every score before top-k."""
        if bias is None:
            if self._bias is not None:                     # (nothing set: nothing to clear -- saves a C call per query)
                self._bias = None
                _check(_lib.hdb_index_set_bias(self._h, None), "hdb_index_set_bias")
            return
        if isinstance(bias, torch.Tensor):
            b = bias.to(self.device, torch.float32).contiguous()
        else:
            b = torch.from_numpy(np.ascontiguousarray(np.asarray(bias, dtype=np.float32))).to(self.device)
        if b.numel() != self.n:
            raise ValueError(f"bias must have {self.n} entries, got {b.numel()}")
        self._bias = b
        _check(_lib.hdb_index_set_bias(self._h, ctypes.c_void_p(b.data_ptr())), "hdb_index_set_bias")

    def set_recency(self, timestamps, recency_bias, ts_max=None, valid=None):
        """bias = recency_bias * exp(ts - max ts) (reference ranking_algorithm.py:183), computed on the
        device in float64 from float64 timestamps, stored as float32.

        ts_max: the maximum to normalise by when it is not the maximum of `timestamps` itself -- the GLOBAL maximum of
        a row-sharded matrix (ShardedIndex.set_recency all-reduces it), or the maximum over the rows that take part
        when a row mask is set.  valid: optional boolean array; the maximum is then taken over those rows only (the
        reference ranks the FILTERED rows, hyperdb.py:1556, so rows a filter removed must not move the maximum)."""
        if timestamps is None or len(timestamps) == 0:
            self.set_bias(None)
            return
        if isinstance(timestamps, torch.Tensor):
            ts = timestamps.to(self.device, torch.float64).contiguous()
            if ts_max is None:
                sel = ts if valid is None else ts[torch.as_tensor(np.asarray(valid, dtype=bool), device=self.device)]
                ts_max = float(sel.max().item()) if sel.numel() else 0.0
        else:
            ts_h = np.ascontiguousarray(np.asarray(timestamps, dtype=np.float64))
            if ts_max is None:
                sel = ts_h if valid is None else ts_h[np.asarray(valid, dtype=bool)]
                ts_max = float(np.max(sel)) if sel.size else 0.0
            ts = torch.from_numpy(ts_h).to(self.device)
        if ts.numel() != self.n:
            raise ValueError(f"operands could not be broadcast together with shapes ({self.n},) ({ts.numel()},)")
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _check(_lib.hdb_recency_bias(ctypes.c_void_p(ts.data_ptr()), self.n, float(recency_bias), float(ts_max),
                                     ctypes.c_void_p(out.data_ptr()), self.device.index or 0,
                                     _stream_ptr(self.device)), "hdb_recency_bias")
        self._bias = out
        _check(_lib.hdb_index_set_bias(self._h, ctypes.c_void_p(out.data_ptr())), "hdb_index_set_bias")

    def recency_twice(self, ts_dev, mask_dev, recency_bias, ts_max, ts_min):
        """Both decays of a HyperDB.query() call (reference hyperdb.py:1344, then ranking_algorithm.py:183) for the rows
        `mask_dev` keeps, from a resident float64 timestamp column: -> float32 CUDA tensor (hdb_recency_bias_twice).
        ts_max / ts_min: newest / oldest timestamp among the kept rows."""
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _check(_lib.hdb_recency_bias_twice(ctypes.c_void_p(ts_dev.data_ptr()),
                                           ctypes.c_void_p(mask_dev.data_ptr()) if mask_dev is not None else None, self.n,
                                           float(recency_bias), float(ts_max), float(ts_min), ctypes.c_void_p(out.data_ptr()),
                                           self.device.index or 0, _stream_ptr(self.device)), "hdb_recency_bias_twice")
        return out

    def _forget_rows(self):
        """The matrix changed: the library dropped the list and the group ids with mask and bias, and nothing validated describes
        the new rows."""
        self._rows = None
        self._rows_ok.clear()
        self._groups, self.n_groups = None, 0
        self._groups_ok.clear()

    def _mask_tensor(self, mask):
        if isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8 and mask.device == self.device and mask.is_contiguous():
            m = mask                                       # a resident 0/1 mask (HyperDB caches them per filter): borrowed as it is
        elif isinstance(mask, torch.Tensor):
            m = (mask != 0).to(self.device, torch.uint8).contiguous()
        else:
            m = torch.from_numpy(np.ascontiguousarray((np.asarray(mask) != 0).astype(np.uint8))).to(self.device)
        if m.numel() != self.n:
            raise ValueError("mask must have one entry per row")
        return m

    def set_row_mask(self, mask):
        """mask: None, or one entry per row (non-zero = the row takes part).  Drops a row list set by set_row_subset."""
        if mask is None:
            if self._mask is not None:
                self._mask = self._rows = None
                _check(_lib.hdb_index_set_row_mask(self._h, None), "hdb_index_set_row_mask")
            return
        m = self._mask_tensor(mask)
        self._mask, self._rows = m, None
        _check(_lib.hdb_index_set_row_mask(self._h, ctypes.c_void_p(m.data_ptr())), "hdb_index_set_row_mask")

    def _row_list(self, rows):
        """numpy / torch -> the validated int64 device list.  One check per list: a resident list that passed before (the facade
        caches its lists per filter) is taken as it is."""
        if isinstance(rows, torch.Tensor) and id(rows) in self._rows_ok:
            self._rows_ok.move_to_end(id(rows))
            return rows
        if isinstance(rows, torch.Tensor):
            h = rows.detach().cpu().numpy()
        else:
            h = np.asarray(rows)
        if h.ndim != 1 or h.size == 0:
            raise ValueError("row list must be a non-empty 1-D array of row ids")
        if h.dtype.kind not in "iu":
            raise ValueError("row list must hold integers")
        h = np.ascontiguousarray(h, dtype=np.int64)
        if int(h[0]) < 0 or int(h[-1]) >= self.n or (h.size > 1 and bool((h[1:] <= h[:-1]).any())):
            raise ValueError(f"row list must be strictly ascending row ids in [0, {self.n})")
        if isinstance(rows, torch.Tensor) and rows.dtype == torch.int64 and rows.device == self.device and rows.is_contiguous():
            r = rows
        else:
            r = torch.from_numpy(h).to(self.device)
        self._rows_ok[id(r)] = r
        while len(self._rows_ok) > HOST_RECORD_SLOTS:
            self._rows_ok.popitem(last=False)
        return r

    def set_row_subset(self, mask, rows):
        """Row mask plus the strictly ascending list of the rows it keeps (hdb_index_set_row_subset): selective filters then read
        only the listed rows where the library's rule says so, every other call uses the mask.  rows: numpy or torch, validated
        here before anything is launched (non-empty, strictly ascending, inside [0, n)): ValueError otherwise.  The caller
        guarantees that list and mask describe the same rows.  rows = None is set_row_mask(mask)."""
        if mask is None or rows is None:
            if mask is None and rows is not None:
                raise ValueError("a row list needs its mask")
            self.set_row_mask(mask)
            return
        r = self._row_list(rows)
        m = self._mask_tensor(mask)
        self._mask, self._rows = m, r
        _check(_lib.hdb_index_set_row_subset(self._h, ctypes.c_void_p(m.data_ptr()), ctypes.c_void_p(r.data_ptr()), int(r.numel())),
               "hdb_index_set_row_subset")

    # -- groups: one id per row, one hit per group ----------------------------------------------
    def set_groups(self, groups, n_groups=None):
        """A group id per row (hdb_index_set_groups) for topk_grouped: numpy or torch, any integer dtype, one entry per row, every
        id in ``[0, n_groups)``; ``n_groups`` defaults to the largest id + 1.  Checked here on the host, once per array and before
        anything is launched: a wrong length, a negative id or an id >= n_groups raises ValueError naming the value.  ``None``
        clears.  append / update / compact drop the ids with mask and bias."""
        if groups is None:
            if self._groups is not None:
                self._groups, self.n_groups = None, 0
                _check(_lib.hdb_index_set_groups(self._h, None, 0), "hdb_index_set_groups")
            return
        g, top = check_groups(groups, self.n, self._groups_ok, self.device)
        ng = top if n_groups is None else int(n_groups)
        if ng < top or ng < 1:
            raise ValueError(f"set_groups: group id {top - 1} is not in [0, {ng}): n_groups is too small")
        self._groups_ok[id(g)] = (g, top)
        while len(self._groups_ok) > HOST_RECORD_SLOTS:
            self._groups_ok.popitem(last=False)
        self._groups, self.n_groups = g, ng
        _check(_lib.hdb_index_set_groups(self._h, ctypes.c_void_p(g.data_ptr()), ng), "hdb_index_set_groups")

    def topk_grouped(self, Q, k, metric_id):
        """One row per group, k distinct groups per query (hdb_topk_grouped_host) -> numpy (int64 [nq,k], float32 [nq,k])
        (copies): each group's best row by (score descending, row ascending), the first k of them; -1 / -inf where fewer than k
        groups can be returned.  Needs set_groups (ValueError otherwise); hamming / jaccard and k > 2048: NotImplementedError."""
        qt = self._query_tensor(Q, batched=True)
        nq, k = int(qt.shape[0]), int(k)
        if nq == 0 or k < 1:
            raise ValueError("topk_grouped: need at least one query and k >= 1")
        slot = self._record_slot(nq, k) if k <= HDB_MAX_K else (None, None)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_topk_grouped_host(self._h, ctypes.c_void_p(qt.data_ptr()), nq, k, int(metric_id), ctypes.c_void_p(slot[1]),
                                              _stream_ptr(self.device)), "hdb_topk_grouped_host")
        if (slot[4] & Q_NAN).any():
            raise ValueError(NAN_MESSAGE)
        return slot[2].copy(), slot[3].copy()

    def maxsim(self, Q, offsets, k, metric_id):
        """Multi-vector queries (hdb_maxsim_host): ``Q`` the flat ``[nv, d]`` vectors of ``ns`` sets, set ``s`` = rows
        ``offsets[s] .. offsets[s + 1]`` (``pack_query_sets`` makes both) -> numpy ``(group ids [ns, k] int64, scores [ns, k]
        float32)`` (copies): the groups by the sum over the set's vectors of each vector's best row in the group, score descending,
        group id ascending; ``-1`` / ``-inf`` where fewer than k groups have an eligible row for every vector.  The status words of
        the call stay in ``maxsim_status`` (Q_BADROW: a group id outside ``[0, n_groups)``).  Needs set_groups (ValueError
        otherwise); a NaN vector raises ValueError; hamming / jaccard and k > 2048: NotImplementedError."""
        qt = self._query_tensor(Q, batched=True)
        off = np.ascontiguousarray(np.asarray(offsets), dtype=np.int32).reshape(-1)
        ns, k = int(off.size) - 1, int(k)
        if ns < 1 or k < 1:
            raise ValueError("maxsim: need at least one query set and k >= 1")
        if int(off[-1]) != int(qt.shape[0]):
            raise ValueError(f"maxsim: offsets end at {int(off[-1])}, the flat matrix holds {int(qt.shape[0])} vectors")
        slot = self._record_slot(ns, k) if k <= HDB_MAX_K else (None, None)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_maxsim_host(self._h, ctypes.c_void_p(qt.data_ptr()), off.ctypes.data_as(ctypes.c_void_p), ns, k, int(metric_id),
                                        ctypes.c_void_p(slot[1]), _stream_ptr(self.device)), "hdb_maxsim_host")
        self.maxsim_status = slot[4].copy()
        if (slot[4] & Q_NAN).any():
            raise ValueError(NAN_MESSAGE)
        return slot[2].copy(), slot[3].copy()

    # -- options / stats -----------------------------------------------------------------------
    def set_option(self, name, value):
        """An option of the index by its C name (include/hyperdb_hip.h lists them), e.g. ``set_option("b1_mfma_min_q", 5)``: a
        storage="bits" index sends dot / cosine / euclidean / pearson batches of 5+ queries to the bf16 matrix cores (d = 128 .. 512,
        and 640 .. 4096 in K slices; 0 = never, the default; ``stat("b1_mfma_min_q")`` is the threshold in force)."""
        _check(_lib.hdb_set_option(self._h, name.encode(), int(value)), "hdb_set_option")

    def stat(self, name):
        v = ctypes.c_int64(0)
        _check(_lib.hdb_get_stat(self._h, name.encode(), ctypes.byref(v)), "hdb_get_stat")
        return int(v.value)

    # -- queries -------------------------------------------------------------------------------
    def _stage_host_query(self, q):
        """A host query batch for a SYNCHRONOUS call: converted once into a cached pinned buffer.  Up to 4 queries are read by
        the kernels straight from that buffer (pinned host memory is device-visible: 1.5 KB per query over PCIe costs less
        than a copy on the stream ahead of the launch); larger batches go through one asynchronous copy into a cached device
        tensor.  (The reference hands numpy queries to numpy: hyperdb.py:1556.)"""
        npdt = np.float64 if self.dtype == HDB_F64 else np.float32
        a = np.asarray(q)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"shapes ({self.n},{self.d}) and {tuple(np.asarray(q).shape)} not aligned")
        nq = int(a.shape[0])
        slot = self._stage_slot(nq, npdt)
        np.copyto(slot[1], a, casting="unsafe")
        if slot[2] is None:
            return slot[0]
        slot[2].copy_(slot[0], non_blocking=True)
        return slot[2]

    def _stage_slot(self, nq, npdt):
        key = (nq, npdt)
        slot = self._qstage.get(key)
        if slot is None:
            pin = torch.empty((nq, self.d), dtype=torch.float64 if npdt is np.float64 else torch.float32, pin_memory=True)
            dev = None if nq <= 4 else torch.empty((nq, self.d), dtype=pin.dtype, device=self.device)
            slot = self._qstage[key] = (pin, pin.numpy(), dev, (pin if dev is None else dev).data_ptr())
            while len(self._qstage) > HOST_RECORD_SLOTS:
                self._qstage.popitem(last=False)
        else:
            self._qstage.move_to_end(key)
        return slot

    def _query_tensor(self, q, batched, staged=False):
        qdt = torch.float64 if self.dtype == HDB_F64 else torch.float32
        if self.dtype == HDB_B1:
            q = self._bits_query(q)
        if staged and batched and not isinstance(q, torch.Tensor):
            return self._stage_host_query(q)
        if isinstance(q, torch.Tensor):
            if batched and q.dtype == qdt and q.dim() == 2 and q.shape[1] == self.d and q.is_contiguous() and \
                    (q.device == self.device or (staged and q.device.type == "cpu" and q.is_pinned())):
                return q                                 # the per-query fast path: nothing to convert (or: already staged)
            t = q.to(self.device, qdt)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(q, dtype=np.float64))).to(self.device, qdt)
        if batched:
            if t.dim() == 1:
                t = t.reshape(1, -1)
            if t.dim() != 2 or t.shape[1] != self.d:
                raise ValueError(f"shapes ({self.n},{self.d}) and {tuple(t.shape)} not aligned")
        else:
            t = t.reshape(-1)
            if t.numel() != self.d:
                raise ValueError(f"shapes ({self.n},{self.d}) and ({t.numel()},) not aligned: "
                                 f"{self.d} (dim 1) != {t.numel()} (dim 0)")
        return t.contiguous()

    def scores(self, q, metric_id):
        """All N scores of one query as a float32 CUDA tensor (no bias, no mask)."""
        qt = self._query_tensor(q, batched=False)
        out = torch.empty(self.n, dtype=torch.float32, device=self.device)
        _check(_lib.hdb_scores(self._h, ctypes.c_void_p(qt.data_ptr()), int(metric_id),
                               ctypes.c_void_p(out.data_ptr()), _stream_ptr(self.device)), "hdb_scores")
        return out

    def topk_device(self, Q, k, metric_id, exact=False):
        """Enqueue the top-k of a (nq, d) query batch; returns CUDA tensors (idx, score, status)."""
        qt = self._query_tensor(Q, batched=True)
        nq = int(qt.shape[0])
        idx = torch.empty((nq, k), dtype=torch.int64, device=self.device)
        sc = torch.empty((nq, k), dtype=torch.float32, device=self.device)
        st = torch.empty((nq,), dtype=torch.int32, device=self.device)
        fn = _lib.hdb_topk_exact if exact else _lib.hdb_topk
        _check(fn(self._h, ctypes.c_void_p(qt.data_ptr()), nq, int(k), int(metric_id),
                  ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(sc.data_ptr()),
                  ctypes.c_void_p(st.data_ptr()), _stream_ptr(self.device)), "hdb_topk")
        return idx, sc, st

    def topk_packed(self, Q, k, metric_id, record, exact=False):
        """Enqueue the top-k of a batch straight into a packed exchange record (uint8 CUDA tensor of
        hdb_packed_bytes(nq, k) bytes): [idx int64][score f32][status i32]."""
        qt = self._query_tensor(Q, batched=True)
        nq = int(qt.shape[0])
        base = record.data_ptr()
        fn = _lib.hdb_topk_exact if exact else _lib.hdb_topk
        _check(fn(self._h, ctypes.c_void_p(qt.data_ptr()), nq, int(k), int(metric_id), ctypes.c_void_p(base),
                  ctypes.c_void_p(base + nq * k * 8), ctypes.c_void_p(base + nq * k * 12),
                  _stream_ptr(self.device)), "hdb_topk")

    def topk_views(self, Q, k, metric_id):
        """One C call (hdb_topk_host): kernels + D2H of the packed record into a cached pinned buffer + sync + the
        rare exact re-run.  Returns numpy VIEWS (idx int64 [nq,k], score float32 [nq,k], status int32 [nq]) that are
        overwritten by the next call of THIS index with the same (nq, k); the record belongs to the index (two
        indices, devices or shard groups never share one) and at most HOST_RECORD_SLOTS shapes are kept."""
        if self.dtype == HDB_B1:
            Q = self._bits_query(Q)
        if type(Q) is np.ndarray and Q.ndim <= 2 and Q.shape[-1] == self.d and Q.size <= 4 * self.d and Q.size:
            # the per-query path of the drop-in entry points (a host query of 1-4 rows): straight into the cached pinned staging
            # buffer the kernels read, no tensor objects, no per-call ctypes wrappers (tools/time_host_path.py)
            nq = Q.size // self.d
            qs = self._stage_slot(nq, np.float64 if self.dtype == HDB_F64 else np.float32)
            np.copyto(qs[1], Q if Q.ndim == 2 else Q.reshape(1, -1), casting="unsafe")
            qptr = qs[3]
        else:
            qt = self._query_tensor(Q, batched=True, staged=True)
            nq, qptr = int(qt.shape[0]), qt.data_ptr()
        k = int(k)
        slot = self._host_records.get((nq, k))
        if slot is None:                                 # pinned record + its numpy views, built once per (nq, k)
            host = torch.empty(packed_bytes(nq, k), dtype=torch.uint8, pin_memory=True)
            h = host.numpy()
            slot = (host, host.data_ptr(), h[:nq * k * 8].view(np.int64).reshape(nq, k),
                    h[nq * k * 8:nq * k * 12].view(np.float32).reshape(nq, k), h[nq * k * 12:nq * k * 12 + nq * 4].view(np.int32), h)
            self._host_records[(nq, k)] = slot
            while len(self._host_records) > HOST_RECORD_SLOTS:
                self._host_records.popitem(last=False)
        elif len(self._host_records) > 1:
            self._host_records.move_to_end((nq, k))
        rc = _lib.hdb_topk_host(self._h, qptr, nq, k, int(metric_id), slot[1], _stream_int(self.device))
        if rc:
            _check(rc, "hdb_topk_host")
        return slot[2], slot[3], slot[4]

    def topk_record_host(self, Q, k, metric_id):
        """topk_views, but returns the whole packed record as ONE uint8 numpy view (what a shard hands to the exchange)."""
        qt = self._query_tensor(Q, batched=True, staged=True)
        nq = int(qt.shape[0])
        self.topk_views(qt, k, metric_id)
        return self._host_records[(nq, int(k))][5]

    # -- rerank: every query against its own list of rows -----------------------------------------
    def _candidates(self, cand, nq):
        """The lists of a rerank call -> (contiguous int64 tensor [nq, m] on the index's device, m); host arrays are range-checked."""
        m = check_candidates(cand, nq, self.n, self.row_base)
        if isinstance(cand, torch.Tensor):
            if cand.device.type != "cpu" and cand.device != self.device:
                raise ValueError(f"candidates live on {cand.device}, the index on {self.device}")
            t = cand.detach().to(self.device, torch.int64)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(cand), dtype=np.int64)).to(self.device)
        return t.contiguous(), m

    def rerank_device(self, Q, cand, k, metric_id):
        """Enqueue the exact top-k of every query among ITS OWN candidates (hdb_rerank): ``cand`` is ``[nq, m]`` global row ids, a
        host array or an int64 CUDA tensor on the index's device; negative ids are padding.  Returns CUDA tensors (idx, score,
        status); the status word of a query is 0, Q_NAN or Q_BADROW (an id outside the index: skipped)."""
        qt = self._query_tensor(Q, batched=True)
        nq = int(qt.shape[0])
        ct, m = self._candidates(cand, nq)
        k = int(k)
        idx = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=self.device)
        sc = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=self.device)
        st = torch.empty((nq,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_rerank(self._h, ctypes.c_void_p(qt.data_ptr()), nq, ctypes.c_void_p(ct.data_ptr()), m, k, int(metric_id),
                                   ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(st.data_ptr()),
                                   _stream_ptr(self.device)), "hdb_rerank")
        return idx, sc, st

    def _record_slot(self, nq, k):
        """The pinned result record of (nq, k) and its numpy views (topk_views keeps the same cache)."""
        slot = self._host_records.get((nq, k))
        if slot is None:
            host = torch.empty(packed_bytes(nq, k), dtype=torch.uint8, pin_memory=True)
            h = host.numpy()
            slot = (host, host.data_ptr(), h[:nq * k * 8].view(np.int64).reshape(nq, k),
                    h[nq * k * 8:nq * k * 12].view(np.float32).reshape(nq, k), h[nq * k * 12:nq * k * 12 + nq * 4].view(np.int32), h)
            self._host_records[(nq, k)] = slot
            while len(self._host_records) > HOST_RECORD_SLOTS:
                self._host_records.popitem(last=False)
        else:
            self._host_records.move_to_end((nq, k))
        return slot

    @staticmethod
    def _raise_rerank_status(st):
        if (st & Q_NAN).any():
            raise ValueError(NAN_MESSAGE)
        if (st & Q_BADROW).any():
            raise IndexError(f"{BADROW_MESSAGE}: the lists of queries {np.flatnonzero(st & Q_BADROW)[:8].tolist()} hold one")

    def rerank(self, Q, cand, k, metric_id):
        """rerank_device through one C call (hdb_rerank_host) -> numpy (int64 [nq,k], float32 [nq,k]) (copies).  Raises ValueError
        on a NaN query and IndexError on a candidate id outside the index."""
        qt = self._query_tensor(Q, batched=True)
        nq = int(qt.shape[0])
        ct, m = self._candidates(cand, nq)
        k = int(k)
        if nq == 0 or k < 1:
            raise ValueError("rerank: need at least one query and k >= 1")
        slot = self._record_slot(nq, k)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_rerank_host(self._h, ctypes.c_void_p(qt.data_ptr()), nq, ctypes.c_void_p(ct.data_ptr()), m, k, int(metric_id),
                                        ctypes.c_void_p(slot[1]), _stream_ptr(self.device)), "hdb_rerank_host")
        self._raise_rerank_status(slot[4])
        return slot[2].copy(), slot[3].copy()

    def two_stage(self, first, Q1, metric1_id, k1, Q2, metric2_id, k):
        """One hdb_two_stage_host call: top-k1 of ``Q1`` on the index ``first``, those ids reranked on THIS index with ``Q2`` ->
        numpy (int64 [nq,k], float32 [nq,k]) (copies).  ValueError when the two handles differ in n, row_base or device."""
        if not isinstance(first, GpuIndex):
            raise NotImplementedError("two_stage: the first stage must be a single GpuIndex")
        if first.n != self.n or first.row_base != self.row_base or first.device != self.device:
            raise ValueError("two_stage: the two indexes must hold the same rows (n, row_base) on the same device")
        q1 = first._query_tensor(Q1, batched=True)
        q2 = self._query_tensor(Q2, batched=True)
        nq = int(q2.shape[0])
        if int(q1.shape[0]) != nq:
            raise ValueError(f"two_stage: {q1.shape[0]} first-stage queries for {nq} queries")
        k, k1 = int(k), int(k1)
        if nq == 0 or k < 1:
            raise ValueError("two_stage: need at least one query and k >= 1")
        slot = self._record_slot(nq, k)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_two_stage_host(first._h, ctypes.c_void_p(q1.data_ptr()), int(metric1_id), k1, self._h,
                                           ctypes.c_void_p(q2.data_ptr()), int(metric2_id), k, nq, ctypes.c_void_p(slot[1]),
                                           _stream_ptr(self.device)), "hdb_two_stage_host")
        self._raise_rerank_status(slot[4])
        return slot[2].copy(), slot[3].copy()

    # -- diverse top-k: maximal marginal relevance over a call's candidates ------------------------
    def mmr_device(self, idx, scores, k, lambda_mult=0.5, pair_metric_id=None, status=None):
        """Enqueue the diverse top-k of ranked lists (hdb_mmr): ``idx`` (int64) / ``scores`` (float32) ``[nq, m]``,
        ``1 <= k <= m <= 2048``, CUDA tensors on the index's device or host arrays -- what topk_device, rerank_device, a two-stage call or
        collapse_groups return goes in as it is.  Pick t >= 1 is the unpicked candidate with the largest
        ``lambda_mult * relevance - (1 - lambda_mult) * max similarity to a pick``; ``pair_metric_id``: dot, cosine (the default) or
        euclidean between stored rows.  ``status``: the lists' int32 status words, whose Q_NAN bits are carried over.  Returns CUDA
        tensors ``(idx [nq, k], scores [nq, k], status [nq])`` IN PICK ORDER, tail ``-1`` / ``-inf``; Q_BADROW: an id outside the
        index was skipped.  ValueError for sizes or a lambda outside [0, 1]; NotImplementedError for another pair metric or a
        ``storage="bits"`` index."""
        it = torch.as_tensor(idx).to(self.device, torch.int64).contiguous()
        st_ = torch.as_tensor(scores).to(self.device, torch.float32).contiguous()
        if it.dim() != 2 or st_.shape != it.shape:
            raise ValueError(f"mmr_device: idx and scores must be 2-D [nq, m] of one shape, got {tuple(it.shape)} and {tuple(st_.shape)}")
        nq, m, k = int(it.shape[0]), int(it.shape[1]), int(k)
        pm = METRIC_IDS["cosine_similarity"] if pair_metric_id is None else int(pair_metric_id)
        out_i = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=self.device)
        out_s = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=self.device)
        if status is None:
            out_st = torch.zeros((nq,), dtype=torch.int32, device=self.device)
        else:
            out_st = torch.as_tensor(status).to(self.device, torch.int32).reshape(-1).clone()
            if int(out_st.numel()) != nq:
                raise ValueError(f"mmr_device: {int(out_st.numel())} status words for {nq} lists")
        with torch.cuda.device(self.device):
            _check(_lib.hdb_mmr(self._h, ctypes.c_void_p(it.data_ptr()), ctypes.c_void_p(st_.data_ptr()), nq, m, k, float(lambda_mult), pm,
                                ctypes.c_void_p(out_i.data_ptr()), ctypes.c_void_p(out_s.data_ptr()), ctypes.c_void_p(out_st.data_ptr()),
                                _stream_ptr(self.device)), "hdb_mmr")
        return out_i, out_s, out_st

    def mmr(self, Q, m, k, metric_id, lambda_mult=0.5, pair_metric_id=None):
        """One C call (hdb_mmr_host): the top-m of every query under ``metric_id`` (mask and bias of the handle applied), then the
        diverse k of those m -> numpy (int64 [nq,k], float32 [nq,k]) (copies), in pick order; the scores are the relevances.
        ``pair_metric_id`` defaults to ``metric_id`` where that is dot, cosine or euclidean, to cosine otherwise.  ValueError on a NaN
        query, on sizes (``1 <= k <= m <= min(n, 2048)``) and on a lambda outside [0, 1]."""
        qt = self._query_tensor(Q, batched=True)
        nq, m, k = int(qt.shape[0]), int(m), int(k)
        if nq == 0:
            raise ValueError("mmr: need at least one query")
        if pair_metric_id is None:
            pair_metric_id = int(metric_id) if int(metric_id) in (0, 1, 2) else METRIC_IDS["cosine_similarity"]
        slot = self._record_slot(nq, k) if 1 <= k <= HDB_MAX_K else (None, None)
        with torch.cuda.device(self.device):
            _check(_lib.hdb_mmr_host(self._h, ctypes.c_void_p(qt.data_ptr()), nq, m, k, int(metric_id), float(lambda_mult), int(pair_metric_id),
                                     ctypes.c_void_p(slot[1]), _stream_ptr(self.device)), "hdb_mmr_host")
        if (slot[4] & Q_NAN).any():
            raise ValueError(NAN_MESSAGE)
        return slot[2].copy(), slot[3].copy()

    def topk(self, Q, k, metric_id):
        """Top-k of a query batch on the host: (int64 [nq,k], float32 [nq,k]) (copies)."""
        idx, sc, st = self.topk_views(Q, k, metric_id)
        if (st[0] & Q_NAN) if len(st) == 1 else (st & Q_NAN).any():      # (one query: a scalar test instead of two array operations)
            raise ValueError(NAN_MESSAGE)
        return idx.copy(), sc.copy()


BADROW_MESSAGE = "candidate id outside the index"


def check_candidates(cand, nq, n, row_base):
    """The candidate lists of a rerank call, checked on the host before any GPU call -> m, the list length.

    ``cand`` is a 2-D integer array or tensor ``[nq, m]`` with ``1 <= m <= 8192`` (ValueError otherwise).  Ids are global (row_base
    added, as top-k calls return them); a negative id is padding.  A HOST array is also range-checked: an id ``>= row_base + n``,
    or a non-negative id below ``row_base``, raises IndexError naming the value.  A device tensor is not read here: the kernels
    skip such an id and say so in the query's status word (Q_BADROW)."""
    if isinstance(cand, torch.Tensor):
        shape, integer, host = tuple(cand.shape), not (cand.dtype.is_floating_point or cand.dtype.is_complex or cand.dtype == torch.bool), None
        if cand.device.type == "cpu":
            host = cand.detach().numpy()
    else:
        host = cand if isinstance(cand, np.ndarray) else np.asarray(cand)
        shape, integer = tuple(host.shape), host.dtype.kind in "iu"
    if len(shape) != 2:
        raise ValueError(f"candidates must be a 2-D array [nq, m], got shape {shape}")
    if not integer:
        raise ValueError("candidates must hold integer row ids")
    if shape[0] != int(nq):
        raise ValueError(f"candidates must have one list per query: {nq} queries, {shape[0]} lists")
    m = int(shape[1])
    if m < 1 or m > CAND_CAP:
        raise ValueError(f"candidates per query must be in [1, {CAND_CAP}], got {m}")
    if host is not None and host.size:
        lo, hi = int(row_base), int(row_base) + int(n)
        bad = (host >= hi) | ((host >= 0) & (host < lo))
        if bad.any():
            raise IndexError(f"{BADROW_MESSAGE}: {int(host[bad].reshape(-1)[0])} is not in [{lo}, {hi})")
    return m


def check_groups(groups, n, seen=None, device=None):
    """The group ids of a set_groups / collapse_groups call, checked on the host -> (int32 tensor, largest id + 1).

    ``groups``: numpy or torch, any integer dtype, 1-D with ``n`` entries, no negative id (ValueError naming the length or the
    offending value otherwise).  ``seen``: the cache of arrays that passed before (id -> (tensor, top)); ``device``: where the
    int32 copy goes (None: it stays on the host)."""
    if seen is not None and isinstance(groups, torch.Tensor) and id(groups) in seen:
        seen.move_to_end(id(groups))
        return seen[id(groups)]
    if isinstance(groups, torch.Tensor):
        if groups.dtype.is_floating_point or groups.dtype.is_complex or groups.dtype == torch.bool:
            raise ValueError(f"group ids must be integers, got {groups.dtype}")
        h = groups.detach().cpu().numpy()
    else:
        h = np.asarray(groups)
        if h.dtype.kind not in "iu":
            raise ValueError(f"group ids must be integers, got dtype {h.dtype}")
    if h.ndim != 1 or h.size != int(n):
        raise ValueError(f"group ids must be 1-D with one entry per row ({int(n)}), got shape {tuple(h.shape)}")
    if h.size == 0:
        raise ValueError("group ids of an empty index")
    lo, hi = int(h.min()), int(h.max())
    if lo < 0:
        raise ValueError(f"group id {lo} is negative: ids must be in [0, n_groups)")
    if hi >= 2 ** 31 - 1:
        raise ValueError(f"group id {hi} does not fit: at most 2^31 - 1 groups")
    if isinstance(groups, torch.Tensor) and groups.dtype == torch.int32 and groups.is_contiguous() and (device is None or groups.device == device):
        g = groups
    else:
        g = torch.from_numpy(np.ascontiguousarray(h, dtype=np.int32))
        if device is not None:
            g = g.to(device)
    return g, hi + 1


def collapse_groups_host(idx, scores, groups, k, row_base=0):
    """The model of hdb_collapse_groups in numpy: ranked lists ``idx`` / ``scores`` ``[nq, m]`` -> ``(idx [nq, k], scores [nq, k],
    status [nq])``: each group's first occurrence in list order, then ``-1`` / ``-inf``.  A negative id or an entry at ``-inf`` is
    padding; an id outside the rows of ``groups`` is skipped and sets Q_BADROW; Q_GROUPS_SHORT: fewer than k groups in a list
    without padding that is shorter than the index."""
    idx = np.asarray(idx, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    groups = np.asarray(groups)
    nq, m = idx.shape
    n, k = int(groups.shape[0]), int(k)
    out_i = np.full((nq, k), -1, np.int64)
    out_s = np.full((nq, k), -np.inf, np.float32)
    status = np.zeros(nq, np.int32)
    for q in range(nq):
        seen, found, pad = set(), 0, False
        for j in range(m):
            r = int(idx[q, j])
            if r < 0 or scores[q, j] == -np.inf:
                pad = True
                continue
            if r < row_base or r - row_base >= n:
                status[q] |= Q_BADROW
                continue
            g = int(groups[r - row_base])
            if g in seen:
                continue
            seen.add(g)
            if found < k:
                out_i[q, found], out_s[q, found] = r, scores[q, j]
            found += 1
        if found < k and not pad and m < n:
            status[q] |= Q_GROUPS_SHORT
    return out_i, out_s, status


def pack_query_sets(x, d):
    """Query sets -> ``(flat float32 [nv, d], int32 offsets [ns + 1])`` for ``GpuIndex.maxsim``.  ``x``: a ``(T, d)`` array (one
    set), an ``(S, T, d)`` array (S sets of T vectors) or a list of ``(T_i, d)`` arrays (ragged sets).  ValueError for an empty set, no
    set at all or a width other than ``d``."""
    d = int(d)
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray) and x.dtype != object:
        if x.ndim == 2:
            sets = [x]
        elif x.ndim == 3:
            sets = [x[i] for i in range(x.shape[0])]
        else:
            raise ValueError(f"query sets must be (T, d), (S, T, d) or a list of (T_i, d) arrays, got shape {tuple(x.shape)}")
    else:
        sets = [t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in x]
    if not sets:
        raise ValueError("query sets: need at least one set")
    flat, off = [], [0]
    for i, t in enumerate(sets):
        if t.ndim != 2:
            raise ValueError(f"query set {i} must be a (T, {d}) array, got shape {tuple(t.shape)}")
        if t.shape[0] == 0:
            raise ValueError(f"query set {i} is empty: a set needs at least one vector")
        if t.shape[1] != d:
            raise ValueError(f"query set {i} has width {t.shape[1]}, the index has {d}")
        flat.append(np.asarray(t, dtype=np.float32))
        off.append(off[-1] + int(t.shape[0]))
    return np.ascontiguousarray(np.concatenate(flat, axis=0)), np.asarray(off, dtype=np.int32)


def _host_scores(V, q, metric):
    """float64 scores of one vector against the rows of V, by the metric's definition (the models' side of a comparison)."""
    V = np.asarray(V, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        if metric == "dot_product":
            return V @ q
        if metric == "cosine_similarity":
            return (V @ q) / (np.linalg.norm(V, axis=1) * np.linalg.norm(q))
        if metric == "euclidean_metric":
            return 1.0 / (1.0 + np.linalg.norm(V - q, axis=1))
        if metric == "manhattan_distance":
            return 1.0 / (1.0 + np.abs(V - q).sum(axis=1))
        if metric == "pearson_correlation":
            Vc = V - V.mean(axis=1, keepdims=True)
            qc = q - q.mean()
            return (Vc @ qc) / (np.linalg.norm(Vc, axis=1) * np.linalg.norm(qc))
    raise ValueError(f"maxsim_host: metric {metric!r} has no multi-vector model")


def maxsim_host(V, query_sets, groups, k, metric, bias=None, mask=None, n_groups=None):
    """The contract of hdb_maxsim_host in numpy, float64: ``(group ids [ns, k] int64, scores [ns, k] float64)``.  For every set the
    group score is the sum over the set's vectors, in vector order, of the maximum over the group's eligible rows of (score + bias); a
    row the mask excludes, a NaN score or a group id outside ``[0, n_groups)`` is ``-inf``; a group without an eligible row, or with a
    term at ``-inf``, scores ``-inf`` and is never returned.  Order: score descending, group id ascending; tail ``-1`` / ``-inf``."""
    V = np.asarray(V)
    n = int(V.shape[0])
    flat, off = pack_query_sets(query_sets, V.shape[1])
    flat = flat.astype(np.float64)
    g = np.asarray(groups).astype(np.int64).reshape(-1)
    if g.size != n:
        raise ValueError(f"maxsim_host: group ids must have one entry per row ({n}), got {g.size}")
    ng = int(n_groups) if n_groups is not None else (int(g.max()) + 1 if n else 0)
    ok = (g >= 0) & (g < ng)
    if mask is not None:
        ok &= np.asarray(mask).reshape(-1) != 0
    b = np.zeros(n) if bias is None else np.asarray(bias, dtype=np.float64).reshape(-1)
    k = int(k)
    ns = int(off.size) - 1
    out_i = np.full((ns, k), -1, dtype=np.int64)
    out_s = np.full((ns, k), -np.inf, dtype=np.float64)
    gi = g[ok]
    for s in range(ns):
        total = None
        for v in range(int(off[s]), int(off[s + 1])):
            x = _host_scores(V, flat[v], metric) + b
            x = np.where(np.isnan(x), -np.inf, x)[ok]
            best = np.full(ng, -np.inf)
            np.maximum.at(best, gi, x)
            with np.errstate(invalid="ignore"):
                total = best if total is None else total + best
        total = np.where(np.isnan(total), -np.inf, total)
        order = np.lexsort((np.arange(ng), -total))
        order = order[total[order] > -np.inf][:k]
        out_i[s, :order.size] = order
        out_s[s, :order.size] = total[order]
    return out_i, out_s


def _pair_matrix_host(X, pair_metric):
    """float64 similarities of every two rows of X by the metric's definition, rounded to float32, NaN -> -inf."""
    c = X.shape[0]
    with np.errstate(all="ignore"):
        if pair_metric == "euclidean_metric":                 # the differences themselves, row by row
            P = np.empty((c, c), np.float64)
            for i in range(c):
                D = X - X[i]
                P[i] = 1.0 / (1.0 + np.sqrt((D * D).sum(axis=1)))
        else:
            P = X @ X.T
            if pair_metric == "cosine_similarity":
                norm = np.sqrt((X * X).sum(axis=1))
                inv = np.where(norm > 0, 1.0 / np.where(norm > 0, norm, 1.0), 1.0)      # (zero norm: 1, as the index's cache)
                P = P * inv[:, None] * inv[None, :]
        P = P.astype(np.float32)
    return np.where(np.isnan(P), np.float32(-np.inf), P)


def mmr_host(V, idx, scores, k, lambda_mult, pair_metric, row_base=0):
    """The contract of hdb_mmr in numpy: ranked lists ``idx`` / ``scores`` ``[nq, m]`` over the rows of ``V`` -> ``(idx [nq, k] int64,
    scores [nq, k] float32, status [nq] int32)`` in pick order, tail ``-1`` / ``-inf``.  A negative id or an entry at ``-inf`` is
    padding; an id outside ``[row_base, row_base + n)`` is skipped and sets Q_BADROW; an id listed twice counts once, at its first
    position.  Step 0 picks the largest relevance; step t the unpicked candidate with the largest
    ``canon(lam * r - (1 - lam) * pen)`` in float32 -- every operation rounded on its own --, ``pen`` the largest pair similarity to
    a pick; ties go to the lowest list position.  Pair similarities (``pair_metric``: a name of PAIR_METRICS or its id) are float64,
    rounded to float32."""
    if not isinstance(pair_metric, str):
        pair_metric = {v: n_ for n_, v in METRIC_IDS.items()}.get(int(pair_metric), pair_metric)
    if pair_metric not in PAIR_METRICS:
        raise NotImplementedError(f"mmr_host: pair metric {pair_metric!r} is not one of {PAIR_METRICS}")
    V = np.asarray(V, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    nq, m = idx.shape
    n, k = int(V.shape[0]), int(k)
    lam = np.float32(lambda_mult)
    oml = np.float32(1.0) - lam
    out_i = np.full((nq, k), -1, np.int64)
    out_s = np.full((nq, k), -np.inf, np.float32)
    status = np.zeros(nq, np.int32)
    for q in range(nq):
        seen, rows, rel = set(), [], []
        for j in range(m):
            r = int(idx[q, j])
            if r < 0 or scores[q, j] == -np.inf:
                continue
            if r < row_base or r - row_base >= n:
                status[q] |= Q_BADROW
                continue
            if r in seen:
                continue
            seen.add(r)
            rows.append(r - row_base)
            rel.append(scores[q, j])
        c = len(rows)
        if c == 0:
            continue
        rows = np.asarray(rows, dtype=np.int64)
        rel = np.asarray(rel, dtype=np.float32)
        rel = np.where(np.isnan(rel), np.float32(-np.inf), rel) + np.float32(0.0)
        P = _pair_matrix_host(V[rows], pair_metric)
        pen = np.full(c, -np.inf, np.float32)
        free = np.ones(c, bool)
        for t in range(min(k, c)):
            if t == 0:
                val = rel
            else:
                with np.errstate(all="ignore"):
                    val = lam * rel - oml * pen
                val = np.where(np.isnan(val), np.float32(-np.inf), val)
            left = np.flatnonzero(free)
            s = int(left[np.argmax(val[left])])               # (argmax: the first of equal values, the lowest position)
            out_i[q, t], out_s[q, t] = rows[s] + row_base, rel[s]
            free[s] = False
            pen = np.maximum(pen, P[s])
    return out_i, out_s, status


def collapse_groups(idx, scores, groups, k, n_groups=None, row_base=0):
    """hdb_collapse_groups on the device: ranked lists ``idx`` (int64) / ``scores`` (float32) ``[nq, m]``, ``1 <= k <= m <= 2048``,
    as CUDA tensors or host arrays, and one group id per row of the index they name (``row_base`` = the id of its row 0) ->
    CUDA tensors ``(idx [nq, k], scores [nq, k], status int32 [nq])``.  The output of topk_device, rerank_device or a two-stage
    call goes in as it is, so grouping composes with those.  Host ``groups`` are checked here (ValueError); a device tensor is
    taken as it is, and the kernel compares every id against ``[0, n_groups)`` before it uses one (Q_BADROW otherwise)."""
    require_gpu()
    if isinstance(idx, torch.Tensor) and idx.is_cuda:
        device = idx.device
    elif isinstance(groups, torch.Tensor) and groups.is_cuda:
        device = groups.device
    else:
        device = torch.device("cuda", torch.cuda.current_device())
    it = torch.as_tensor(idx).to(device, torch.int64).contiguous()
    st_ = torch.as_tensor(scores).to(device, torch.float32).contiguous()
    if it.dim() != 2 or st_.shape != it.shape:
        raise ValueError(f"collapse_groups: idx and scores must be 2-D [nq, m] of one shape, got {tuple(it.shape)} and {tuple(st_.shape)}")
    nq, m, k = int(it.shape[0]), int(it.shape[1]), int(k)
    if isinstance(groups, torch.Tensor) and groups.is_cuda:
        if groups.dtype != torch.int32 or groups.dim() != 1 or not groups.is_contiguous() or groups.device != device:
            raise ValueError("collapse_groups: device group ids must be a contiguous 1-D int32 tensor on the lists' device")
        if n_groups is None:
            raise ValueError("collapse_groups: device group ids need n_groups")
        g, ng = groups, int(n_groups)
    else:
        g, top = check_groups(groups, len(groups), None, device)
        ng = top if n_groups is None else int(n_groups)
        if ng < top:
            raise ValueError(f"collapse_groups: group id {top - 1} is not in [0, {ng}): n_groups is too small")
    out_i = torch.empty((nq, max(k, 0)), dtype=torch.int64, device=device)
    out_s = torch.empty((nq, max(k, 0)), dtype=torch.float32, device=device)
    status = torch.zeros((nq,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        _check(_lib.hdb_collapse_groups(ctypes.c_void_p(it.data_ptr()), ctypes.c_void_p(st_.data_ptr()), nq, m, k, ctypes.c_void_p(g.data_ptr()),
                                        ng, int(g.numel()), int(row_base), ctypes.c_void_p(out_i.data_ptr()), ctypes.c_void_p(out_s.data_ptr()),
                                        ctypes.c_void_p(status.data_ptr()), device.index or 0, _stream_ptr(device)), "hdb_collapse_groups")
    return out_i, out_s, status


def quant_mode(mode):
    """Library code of a ``quantize=`` argument: None or "int8"; anything else raises ValueError."""
    if mode is not None and not isinstance(mode, str):
        raise ValueError(f"quantize must be None or 'int8', got {mode!r}")
    if mode not in QUANT_MODES:
        raise ValueError(f"quantize must be None or 'int8', got {mode!r}")
    return QUANT_MODES[mode]


def request_shadow(index, mode):
    """What a ``quantize=`` argument of an entry point (register_vectors, HyperDB) does with its GpuIndex or GpuGroup: the
    caller asked for a shadow by name, so a bfloat16 index -- every shard of a group -- gets the option ``bf16_quant`` first
    (without it hdb_index_quantize refuses bfloat16 matrices: GpuIndex.quantize).  Other dtypes: quantize(mode) and nothing else."""
    if quant_mode(mode) != HDB_QUANT_NONE and index.dtype == HDB_BF16:
        index.set_option("bf16_quant", 1)
    index.quantize(mode)


def packed_bytes(nq, k):
    return int(_lib.hdb_packed_bytes(int(nq), int(k)))


HOST_RECORD_SLOTS = 8      # pinned result records kept per index / per staging owner (LRU)


def record_to_host(record, nq, k, cache):
    """ONE D2H copy of a packed record (pinned staging buffer from `cache`, an OrderedDict owned by the caller and
    keyed by size) -> numpy views (idx int64 [nq,k], score float32 [nq,k], status int32 [nq]).  Views alias the
    staging buffer: callers copy what they keep."""
    nb = record.numel()
    host = cache.get(nb)
    if host is None:
        host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
        cache[nb] = host
        while len(cache) > HOST_RECORD_SLOTS:
            cache.popitem(last=False)
    else:
        cache.move_to_end(nb)
    host.copy_(record, non_blocking=True)
    torch.cuda.current_stream(record.device).synchronize()
    h = host.numpy()
    idx = h[:nq * k * 8].view(np.int64).reshape(nq, k)
    sc = h[nq * k * 8:nq * k * 12].view(np.float32).reshape(nq, k)
    st = h[nq * k * 12:nq * k * 12 + nq * 4].view(np.int32)
    return idx, sc, st


def record_views(h, nq, k):
    """numpy views (idx int64 [nq,k], score float32 [nq,k], status int32 [nq]) of a packed record held in a uint8 array."""
    return (h[:nq * k * 8].view(np.int64).reshape(nq, k), h[nq * k * 8:nq * k * 12].view(np.float32).reshape(nq, k),
            h[nq * k * 12:nq * k * 12 + nq * 4].view(np.int32))


def merge_topk_host(records, parts, nq, k, out):
    """hdb_merge_topk_host: `records` = parts packed records back to back in HOST memory (uint8 numpy), `out` = uint8
    numpy of packed_bytes(nq, k).  Pure host code (no GPU call).  Returns the views of `out`."""
    nb = packed_bytes(nq, k)
    if records.dtype != np.uint8 or records.size < parts * nb or out.dtype != np.uint8 or out.size < nb:
        raise ValueError("merge_topk_host: records / out must be uint8 arrays of parts * packed_bytes / packed_bytes")
    if not (records.flags["C_CONTIGUOUS"] and out.flags["C_CONTIGUOUS"]):
        raise ValueError("merge_topk_host: contiguous arrays only")
    _check(_lib.hdb_merge_topk_host(ctypes.c_void_p(records.ctypes.data), int(parts), int(nq), int(k),
                                    ctypes.c_void_p(out.ctypes.data)), "hdb_merge_topk_host")
    return record_views(out, nq, k)


def host_exchange_merge(shm_addr, stride, world, rank, seq, record_addr, nq, k, out_addr, timeout_s):
    """hdb_host_exchange_merge on raw addresses (the caller caches them: this sits on the per-query path)."""
    _check(_lib.hdb_host_exchange_merge(shm_addr, stride, world, rank, seq, record_addr, nq, k, out_addr, timeout_s),
           "hdb_host_exchange_merge")


def merge_topk_packed_into(gathered, parts, nq, k, out_record):
    """Merge `parts` gathered records into another packed record (same layout)."""
    base = out_record.data_ptr()
    device = gathered.device
    _check(_lib.hdb_merge_topk_packed(ctypes.c_void_p(gathered.data_ptr()), int(parts), int(nq), int(k),
                                      ctypes.c_void_p(base), ctypes.c_void_p(base + nq * k * 8),
                                      ctypes.c_void_p(base + nq * k * 12), device.index or 0, _stream_ptr(device)),
           "hdb_merge_topk_packed")


def merge_topk_packed(gathered, parts, nq, k):
    """Merge `parts` gathered exchange records (one uint8 CUDA tensor) -> (idx, score, status) CUDA tensors."""
    device = gathered.device
    idx = torch.empty((nq, k), dtype=torch.int64, device=device)
    sc = torch.empty((nq, k), dtype=torch.float32, device=device)
    st = torch.empty((nq,), dtype=torch.int32, device=device)
    _check(_lib.hdb_merge_topk_packed(ctypes.c_void_p(gathered.data_ptr()), int(parts), int(nq), int(k),
                                      ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(sc.data_ptr()),
                                      ctypes.c_void_p(st.data_ptr()), device.index or 0, _stream_ptr(device)),
           "hdb_merge_topk_packed")
    return idx, sc, st


def merge_topk(idx_parts, score_parts, k):
    """Merge all-gathered per-shard lists: idx_parts [parts, nq, k] int64, score_parts float32."""
    parts, nq, kk = (int(x) for x in idx_parts.shape)
    assert kk == k and score_parts.shape == idx_parts.shape
    device = idx_parts.device
    idx = torch.empty((nq, k), dtype=torch.int64, device=device)
    sc = torch.empty((nq, k), dtype=torch.float32, device=device)
    ip, sp = idx_parts.contiguous(), score_parts.contiguous()
    _check(_lib.hdb_merge_topk(ctypes.c_void_p(ip.data_ptr()), ctypes.c_void_p(sp.data_ptr()), parts, nq, k,
                               ctypes.c_void_p(idx.data_ptr()), ctypes.c_void_p(sc.data_ptr()),
                               device.index or 0, _stream_ptr(device)), "hdb_merge_topk")
    return idx, sc
