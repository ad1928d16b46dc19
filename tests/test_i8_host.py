"""CPU-side checks of int8 storage (storage="int8", HDB_I8 = 7): the dtype codes, the host conversion to_i8 (integers in
[-128, 127] or ValueError -- no rounding, scaling or saturation), the upload policy with and without the keyword, the facade's
keyword, and the C ABI's dtype check.  No compute is launched."""
import ctypes

import pytest


def test_codes():
    import torch
    from hyperdb import _native
    assert _native.HDB_I8 == 7
    assert (_native.HDB_F16, _native.HDB_F32, _native.HDB_F64, _native.HDB_BF16, _native.HDB_F8E4M3) == (0, 1, 2, 3, 5)      # the older codes stay
    assert torch.int8 not in _native._TORCH2HDB                    # an int8 tensor is NOT stored natively unless asked for
    assert _native._STORED2HDB[torch.int8] == 7
    for code in (4, 6, 9):
        assert code not in _native._STORED2HDB.values()


def test_to_i8_takes_integers_in_range_only():
    import numpy as np
    import torch
    from hyperdb import _native
    a = np.array([[-128, -1, 0, 1, 127], [5, 6, 7, 8, 9]], dtype=np.int8)
    t = _native.to_i8(a)
    assert t.dtype == torch.int8 and np.array_equal(t.numpy(), a)
    for dt in (np.int64, np.int16, np.float32, np.float64, np.float16, np.uint8):
        src = a.astype(dt) if dt is not np.uint8 else np.abs(a).clip(0, 127).astype(dt)
        got = _native.to_i8(src)
        assert got.dtype == torch.int8 and np.array_equal(got.numpy().astype(np.int64), src.astype(np.int64))
    assert np.array_equal(_native.to_i8([[1, 2], [-3, 4]]).numpy(), np.array([[1, 2], [-3, 4]], dtype=np.int8))      # lists too
    assert np.array_equal(_native.to_i8(torch.tensor([[1.0, -128.0]], dtype=torch.bfloat16)).numpy(), np.array([[1, -128]], dtype=np.int8))
    ti = torch.from_numpy(a)
    assert _native.to_i8(ti) is ti                                  # an int8 tensor goes in as it is
    for bad, name in ((127.5, "127.5"), (128, "128"), (-129, "-129"), (float("nan"), "nan"), (float("inf"), "inf"), (0.5, "0.5")):
        x = np.array([[1.0, 2.0], [bad, 3.0]], dtype=np.float64)
        with pytest.raises(ValueError, match=name):
            _native.to_i8(x)
        with pytest.raises(ValueError, match=name):
            _native.to_i8(torch.from_numpy(x))
    with pytest.raises(ValueError, match="128"):
        _native.to_i8(np.array([[128]], dtype=np.int64))
    with pytest.raises(ValueError, match="200"):
        _native.to_i8(np.array([[200]], dtype=np.uint8))
    with pytest.raises(ValueError):
        _native.to_i8(np.array([["a"]]))


def test_upload_policy_with_and_without_the_keyword():
    import numpy as np
    import torch
    from hyperdb import _native
    cpu = torch.device("cpu")
    src = torch.arange(-16, 16, dtype=torch.int8).reshape(4, 8)
    # without the keyword nothing changes: integers, torch.int8 included, widen to float64
    assert _native.to_device_matrix(src, cpu).dtype == torch.float64
    assert _native.to_device_matrix(src.numpy(), cpu).dtype == torch.float64
    assert _native.to_device_matrix(src, cpu, None).dtype == torch.float64
    # with it the bytes are the matrix
    t = _native.to_device_matrix(src, cpu, "int8")
    assert t.dtype == torch.int8 and t.element_size() == 1 and t.is_contiguous() and torch.equal(t, src)
    tt = _native.to_device_matrix(src.t(), cpu, "int8")
    assert tt.is_contiguous() and torch.equal(tt, src.t().contiguous())
    assert torch.equal(_native.to_device_matrix(src.numpy().astype(np.float32), cpu, "int8"), src)
    with pytest.raises(ValueError, match="0.5"):
        _native.to_device_matrix(np.array([[0.5, 1.0]]), cpu, "int8")
    for bad in ("int4", "uint8", 8, "float8"):
        with pytest.raises(ValueError, match="storage"):
            _native.to_device_matrix(src, cpu, bad)
        with pytest.raises(ValueError, match="storage"):
            _native.GpuIndex(src, storage=bad)                      # (refused before a device is asked for)
    # the float dtypes keep their policy
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.float16), cpu).dtype == torch.float16
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.float8_e4m3fn), cpu).dtype == torch.float8_e4m3fn


def test_result_dtype_follows_the_stored_dtype():
    import numpy as np
    import torch
    import hyperdb.ranking_algorithm as ranking
    assert ranking._STORED2NP[torch.int8] is np.float32            # an int8 index answers in float32 ...
    assert torch.int8 not in ranking._TORCH2NP                     # ... a raw int8 tensor becomes a float64 index and answers in float64
    assert ranking._TORCH2NP.get(torch.int8, np.float64) is np.float64


def test_facade_takes_the_keyword_and_a_bad_add_stores_nothing():
    import numpy as np
    from hyperdb import HyperDB
    db = HyperDB(storage="int8")
    assert db.i8 and db.storage == "int8" and db.fp_precision is np.float32 and db.vectors is None and not db.bf16 and not db.f8
    assert not HyperDB().i8 and HyperDB().storage is None
    with pytest.raises(ValueError):
        HyperDB(fp_precision="int8")                                # still no floating-point precision of that name
    with pytest.raises(ValueError, match="storage"):
        HyperDB(storage="uint8")
    with pytest.raises(ValueError):
        HyperDB(storage="int8", fp_precision="float16")
    with pytest.raises(NotImplementedError):
        HyperDB(storage="int8", quantize="int8")
    # an offending value is refused before anything reaches a device or the document list (no GPU is needed to see it)
    with pytest.raises(ValueError, match="127.5"):
        db.add(["a", "b"], np.array([[1.0, 2.0], [127.5, 0.0]], dtype=np.float32))
    with pytest.raises(ValueError, match="-129"):
        db.add(["a"], np.array([[-129, 0]], dtype=np.int64))
    with pytest.raises(ValueError):
        db.add(["a"], np.array([[np.nan, 0.0]]))
    assert db.documents == [] and db.source_indices == [] and db._index is None


def test_abi_version_and_dtype_check():
    from hyperdb import _native
    lib = _native.lib()
    assert lib.hdb_version() >= 107
    h = ctypes.c_void_p()
    # dtype 7 passes the dtype check: a row too wide for the query tile is refused by the check that FOLLOWS it (no device is touched
    # either way), while the same call with an unassigned code stops at the dtype
    rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000, 7, 0, 0, None)
    assert rc == -1 and b"dtype" not in lib.hdb_last_error() and b"d too large" in lib.hdb_last_error()
    for bad in (4, 6, 9, -1):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000, bad, 0, 0, None)
        assert rc == -1 and b"dtype" in lib.hdb_last_error()
