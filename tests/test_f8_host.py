"""CPU-side checks of the float8 e4m3 storage dtype: the dtype tables of the shim, the upload policy (a torch.float8_e4m3fn tensor
stays one byte per element instead of being widened to float64), the host conversion of float data, the facade's
``fp_precision="float8_e4m3fn"`` with its range check, and the C ABI's dtype check.  No compute is launched."""
import ctypes

import pytest


def test_dtype_tables_carry_float8():
    import numpy as np
    import torch
    from hyperdb import _native
    import hyperdb.ranking_algorithm as ranking
    assert _native.HDB_F8E4M3 == 5
    assert _native._TORCH2HDB[torch.float8_e4m3fn] == 5
    assert (_native.HDB_F16, _native.HDB_F32, _native.HDB_F64, _native.HDB_BF16) == (0, 1, 2, 3)      # the existing codes stay
    assert 4 not in _native._TORCH2HDB.values()                                                    # code 4 stays unassigned
    assert ranking._TORCH2NP[torch.float8_e4m3fn] is np.float32                                    # score vectors come back as float32
    assert _native.F8_MAX == 448.0


def test_upload_keeps_a_float8_tensor_at_one_byte():
    import torch
    from hyperdb import _native
    src = torch.arange(32, dtype=torch.uint8).reshape(4, 8).view(torch.float8_e4m3fn)
    t = _native.to_device_matrix(src, torch.device("cpu"))
    assert t.dtype == torch.float8_e4m3fn and t.element_size() == 1 and t.is_contiguous()
    assert torch.equal(t.view(torch.uint8), src.view(torch.uint8))                                 # the bytes as they were
    # a non-contiguous view arrives contiguous with the same values
    tt = _native.to_device_matrix(src.t(), torch.device("cpu"))
    assert tt.is_contiguous() and torch.equal(tt.view(torch.uint8), src.view(torch.uint8).t().contiguous())
    # the other dtypes keep their policy: float16 / bfloat16 stay, integers widen to float64
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.float16), torch.device("cpu")).dtype == torch.float16
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.bfloat16), torch.device("cpu")).dtype == torch.bfloat16
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.int32), torch.device("cpu")).dtype == torch.float64


def test_host_conversion_is_torchs_own():
    import numpy as np
    import torch
    from hyperdb import _native
    x = np.array([[0.0, -0.0, 1.0, 1.0625, 1.1875, 447.0, 448.0, 464.0, 465.0, 500.0, -500.0, 2.0 ** -9, 2.0 ** -10, 3e-4]], dtype=np.float32)
    got = _native.to_f8(x)
    want = torch.from_numpy(x).to(torch.float8_e4m3fn)
    assert got.dtype == torch.float8_e4m3fn and torch.equal(got.view(torch.uint8), want.view(torch.uint8))
    w = got.float().numpy()[0]
    assert w[3] == 1.0 and w[4] == 1.25                                    # ties go to the even mantissa
    assert w[5] == 448.0 and w[6] == 448.0 and w[7] == 448.0               # up to 464 rounds to 448 ...
    assert np.isnan(w[8]) and np.isnan(w[9]) and np.isnan(w[10])           # ... anything beyond becomes NaN: torch does not saturate
    assert w[11] == 2.0 ** -9 and w[12] == 0.0                             # the smallest subnormal; half of it rounds to even (zero)
    # float64, float16 and torch inputs take the same road; a float8 tensor passes through untouched
    assert torch.equal(_native.to_f8(x.astype(np.float64)).view(torch.uint8), want.view(torch.uint8))
    assert _native.to_f8(want) is want


def test_facade_accepts_float8_precision_and_checks_the_range():
    import numpy as np
    from hyperdb import HyperDB
    db = HyperDB(fp_precision="float8_e4m3fn")
    assert db.fp_precision is np.float32 and db.vectors is None and db.f8 and not db.bf16      # host arrays are the float32 widening
    assert HyperDB(fp_precision="bfloat16").bf16 and not HyperDB(fp_precision="bfloat16").f8
    for name in ("float16", "float32", "float64"):
        assert HyperDB(fp_precision=name).fp_precision is getattr(np, name)
    for bad in ("int8", "bf16", "float8", "float8_e5m2", "fp8"):
        with pytest.raises(ValueError):
            HyperDB(fp_precision=bad)
    # a finite value beyond the range is refused before anything reaches a device (no GPU is needed to see it)
    with pytest.raises(ValueError, match="448"):
        db.add(["a", "b"], np.array([[1.0, 2.0], [500.0, 0.5]], dtype=np.float32))
    with pytest.raises(ValueError, match="[Ss]cale"):
        db.add(["a"], np.array([[-449.0, 0.0]], dtype=np.float64))
    assert db.documents == [] and db._index is None


def test_abi_version_and_dtype_check():
    from hyperdb import _native
    lib = _native.lib()
    assert lib.hdb_version() >= 104
    h = ctypes.c_void_p()
    for bad in (9, 4, -1, 6):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 4, bad, 0, 0, None)
        assert rc == -1 and b"dtype" in lib.hdb_last_error()
    # dtype 5 passes the dtype check: a row too wide for the query tile is refused by the check that FOLLOWS it (no device is touched
    # either way), while the same call with an unassigned code stops at the dtype
    rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000, 5, 0, 0, None)
    assert rc == -1 and b"dtype" not in lib.hdb_last_error() and b"d too large" in lib.hdb_last_error()
    rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000, 4, 0, 0, None)
    assert rc == -1 and b"dtype" in lib.hdb_last_error()
