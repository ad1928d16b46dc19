"""CPU-side checks of the bfloat16 storage dtype: the dtype tables of the shim, the upload policy (a torch.bfloat16 tensor stays
2 bytes per element instead of being widened to float64), the facade's ``fp_precision="bfloat16"`` and the C ABI's dtype check.
No compute is launched."""
import ctypes

import pytest


def test_dtype_tables_carry_bfloat16():
    import numpy as np
    import torch
    from hyperdb import _native
    import hyperdb.ranking_algorithm as ranking
    assert _native.HDB_BF16 == 3
    assert _native._TORCH2HDB[torch.bfloat16] == 3
    assert (_native.HDB_F16, _native.HDB_F32, _native.HDB_F64) == (0, 1, 2)          # the existing codes stay
    assert ranking._TORCH2NP[torch.bfloat16] is np.float32                            # score vectors come back as float32


def test_upload_keeps_a_bfloat16_tensor_as_it_is():
    import torch
    from hyperdb import _native
    t = _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.bfloat16), torch.device("cpu"))
    assert t.dtype == torch.bfloat16 and t.element_size() == 2 and t.is_contiguous()
    # the other dtypes keep their policy: float16 stays, integers widen to float64
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.float16), torch.device("cpu")).dtype == torch.float16
    assert _native.to_device_matrix(torch.zeros(4, 8, dtype=torch.int32), torch.device("cpu")).dtype == torch.float64


def test_facade_accepts_bfloat16_precision():
    import numpy as np
    from hyperdb import HyperDB
    db = HyperDB(fp_precision="bfloat16")
    assert db.fp_precision is np.float32 and db.vectors is None                       # host arrays are the float32 widening
    for name in ("float16", "float32", "float64"):
        assert HyperDB(fp_precision=name).fp_precision is getattr(np, name)
    with pytest.raises(ValueError):
        HyperDB(fp_precision="int8")
    with pytest.raises(ValueError):
        HyperDB(fp_precision="bf16")


def test_abi_version_and_dtype_check():
    from hyperdb import _native
    lib = _native.lib()
    assert lib.hdb_version() >= 103
    h = ctypes.c_void_p()
    for bad in (9, 4, -1):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 4, bad, 0, 0, None)
        assert rc == -1 and b"dtype" in lib.hdb_last_error()
