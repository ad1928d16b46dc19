"""CPU-side checks of packed-bit storage (storage="bits", HDB_B1 = 10): the dtype codes, pack_bits against np.packbits in both bit
orders, the byte-wise big <-> little conversion, the input policy of a bits index (packed uint8 or unpacked bool, nothing else --
no silent binarisation), the policy without the keyword, the refusals of what is not built, and the C ABI's dtype and width
checks.  No compute is launched."""
import ctypes

import numpy as np
import pytest


def test_codes():
    import torch
    from hyperdb import _native
    assert _native.HDB_B1 == 10 and "bits" in _native.STORAGE_MODES and None in _native.STORAGE_MODES and "int8" in _native.STORAGE_MODES
    assert (_native.HDB_F16, _native.HDB_F32, _native.HDB_F64, _native.HDB_BF16, _native.HDB_F8E4M3, _native.HDB_I8) == (0, 1, 2, 3, 5, 7)
    assert torch.uint8 not in _native._TORCH2HDB                    # a uint8 tensor is NOT stored as bits unless asked for
    assert _native._STORED2HDB[torch.uint8] == 10
    for code in (4, 6, 8, 9):
        assert code not in _native._STORED2HDB.values()
    assert _native.storage_mode("bits") == "bits"
    for bad in ("bit", "uint8", "binary", 1):
        with pytest.raises(ValueError, match="storage"):
            _native.storage_mode(bad)


def test_pack_bits_is_packbits_of_x_gt_0():
    import torch
    from hyperdb import _native
    rng = np.random.default_rng(5)
    X = rng.normal(size=(37, 96)).astype(np.float32)
    X[3] = 0.0
    X[4, :10] = -0.0
    for order in ("big", "little"):
        want = np.packbits(X > 0, axis=1, bitorder=order)
        for src in (X, X.astype(np.float64), X.astype(np.float16), torch.from_numpy(X), torch.from_numpy(X).to(torch.bfloat16),
                    (X * 100).astype(np.int64), X > 0, (X > 0).astype(np.uint8), (X > 0).astype(np.int8)):
            if isinstance(src, torch.Tensor) and src.dtype == torch.bfloat16:
                ref = np.packbits(src.float().numpy() > 0, axis=1, bitorder=order)
            elif isinstance(src, np.ndarray) and src.dtype == np.int64:
                ref = np.packbits(src > 0, axis=1, bitorder=order)
            elif isinstance(src, np.ndarray) and src.dtype == np.float16:
                ref = np.packbits(src > 0, axis=1, bitorder=order)
            else:
                ref = want
            got = _native.pack_bits(src, bitorder=order)
            assert got.dtype == np.uint8 and got.shape == (37, 12) and np.array_equal(got, ref)
    assert np.array_equal(_native.pack_bits(X), np.packbits(X > 0, axis=1))      # "big" is the default, as np.packbits has it
    for bad_d in (1, 8, 48, 100):
        with pytest.raises(ValueError, match="multiple of 32"):
            _native.pack_bits(np.zeros((4, bad_d), dtype=np.float32))
    with pytest.raises(ValueError, match="2-D"):
        _native.pack_bits(np.zeros(64, dtype=np.float32))
    with pytest.raises(ValueError, match="bitorder"):
        _native.pack_bits(X, bitorder="msb")
    with pytest.raises(ValueError):
        _native.pack_bits(np.array([["a"] * 32]))


def test_big_little_conversion_on_cpu_tensors():
    import torch
    from hyperdb import _native
    every = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    rev = _native.reverse_bits8(every)
    assert rev.dtype == torch.uint8 and rev.shape == every.shape
    want = np.array([int(f"{b:08b}"[::-1], 2) for b in range(256)], dtype=np.uint8)
    assert np.array_equal(rev.numpy(), want)
    assert torch.equal(_native.reverse_bits8(rev), every)           # an involution
    rng = np.random.default_rng(6)
    bits = rng.random((9, 64)) < 0.5
    big, little = np.packbits(bits, axis=1, bitorder="big"), np.packbits(bits, axis=1, bitorder="little")
    assert np.array_equal(_native.reverse_bits8(torch.from_numpy(big)).numpy(), little)
    # what the device holds is the little order whatever came in; read as little-endian words, element e is bit e & 31 of word e >> 5
    cpu = torch.device("cpu")
    for src, order in ((big, "big"), (little, "little"), (torch.from_numpy(big), "big"), (bits, "big"), (bits, "little"),
                       (torch.from_numpy(bits), "big")):
        t = _native.to_bits(src, cpu, order)
        assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (9, 8) and np.array_equal(t.numpy(), little), order
    words = _native.to_bits(big, cpu, "big").numpy().view("<u4")
    for e in (0, 1, 7, 8, 31, 32, 33, 63):
        assert np.array_equal((words[:, e >> 5] >> (e & 31)) & 1, bits[:, e].astype(np.uint32)), e
    assert np.array_equal(_native.unpack_bits_host(big, "big"), bits.astype(np.float32))
    assert np.array_equal(_native.unpack_bits_host(little, "little"), bits.astype(np.float32))
    t = torch.from_numpy(big.copy())
    _native.to_bits(t, cpu, "big")
    assert np.array_equal(t.numpy(), big)                           # the caller's tensor is not modified


def test_input_policy_packed_uint8_or_bool_only():
    import torch
    from hyperdb import _native
    cpu = torch.device("cpu")
    ok_packed = np.zeros((5, 12), dtype=np.uint8)
    ok_bool = np.zeros((5, 96), dtype=bool)
    assert tuple(_native.to_bits(ok_packed, cpu).shape) == (5, 12) and tuple(_native.to_bits(ok_bool, cpu).shape) == (5, 12)
    assert tuple(_native.to_bits(torch.from_numpy(ok_packed), cpu).shape) == (5, 12)
    bad = (np.zeros((5, 96), dtype=np.float32), np.zeros((5, 96), dtype=np.float64), np.zeros((5, 96), dtype=np.int64),
           np.zeros((5, 96), dtype=np.int8), torch.zeros(5, 96), torch.zeros(5, 96, dtype=torch.int8),
           np.zeros(12, dtype=np.uint8), np.zeros(96, dtype=bool), np.zeros((2, 5, 12), dtype=np.uint8),
           np.zeros((5, 6), dtype=np.uint8),                        # 48 bits per row
           np.zeros((5, 48), dtype=bool), np.zeros((5, 0), dtype=np.uint8), [[0.5] * 32])
    for x in bad:
        with pytest.raises(ValueError, match="pack_bits"):
            _native.to_bits(x, cpu)
        with pytest.raises(ValueError, match="pack_bits"):
            _native.GpuIndex(x, storage="bits")                     # (refused before a device is asked for)
    with pytest.raises(ValueError, match="bitorder"):
        _native.GpuIndex(ok_packed, storage="bits", bitorder="lsb")


def test_uint8_without_the_keyword_is_still_float64():
    import torch
    from hyperdb import _native
    import hyperdb.ranking_algorithm as ranking
    cpu = torch.device("cpu")
    src = np.arange(48, dtype=np.uint8).reshape(4, 12)
    for x in (src, torch.from_numpy(src)):
        for args in ((x, cpu), (x, cpu, None)):
            t = _native.to_device_matrix(*args)
            assert t.dtype == torch.float64 and tuple(t.shape) == (4, 12) and np.array_equal(t.numpy(), src.astype(np.float64))
    assert np.array_equal(_native.to_device_matrix(src > 3, cpu).numpy(), (src > 3).astype(np.float64))
    assert ranking._STORED2NP[torch.uint8] is np.float32             # a bits index answers in float32 ...
    assert torch.uint8 not in ranking._TORCH2NP                      # ... a raw uint8 tensor becomes a float64 index and answers in float64
    assert ranking._TORCH2NP.get(torch.uint8, np.float64) is np.float64


def test_what_is_not_built_says_so():
    from hyperdb import HyperDB, _native
    from hyperdb.group import GpuGroup
    import hyperdb.ranking_algorithm as ranking
    packed = np.zeros((8, 4), dtype=np.uint8)
    with pytest.raises(NotImplementedError, match="single index"):
        ranking.register_vectors(packed, devices=[0], storage="bits")
    with pytest.raises(NotImplementedError, match="single index"):
        GpuGroup(packed, [0], storage="bits")
    with pytest.raises(NotImplementedError, match="single index"):
        HyperDB(storage="bits")
    assert "single index" in _native.BITS_SINGLE_INDEX


def test_abi_version_dtype_and_width_checks():
    from hyperdb import _native
    lib = _native.lib()
    assert lib.hdb_version() >= 108
    h = ctypes.c_void_p()
    # dtype 10 passes the dtype check: a row too wide for the query tile is refused by the check that FOLLOWS it (no device is touched
    # either way), while the same call with an unassigned code stops at the dtype
    rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000 * 32, 10, 0, 0, None)
    assert rc == -1 and b"dtype" not in lib.hdb_last_error() and b"d too large" in lib.hdb_last_error()
    for bad in (4, 6, 8, 9, -1, 11):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000 * 32, bad, 0, 0, None)
        assert rc == -1 and b"dtype" in lib.hdb_last_error()
    # d counts bits and must be a multiple of 32
    for bad_d in (48, 1, 100, 33):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, bad_d, 10, 0, 0, None)
        assert rc == -1 and b"multiple of 32" in lib.hdb_last_error(), bad_d
