"""CPU-side checks of MXFP4 storage (storage="mxfp4", HDB_MXF4 = 13): values, to_mxfp4, row layout, input policy, C ABI.  No compute."""
import ctypes

import numpy as np
import pytest

MAGS = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def _block(codes32, scale):                   # one row of one MX block: the even element in the low nibble
    c = np.asarray(codes32, dtype=np.uint8)
    return (c[0::2] | (c[1::2] << 4)).reshape(1, 16), np.array([[scale]], dtype=np.uint8)


def test_all_codes_widen_to_the_table_exactly():
    from hyperdb import _native
    assert _native.HDB_MXF4 == 13 and "mxfp4" in _native.STORAGE_MODES and _native.storage_mode("mxfp4") == "mxfp4"
    for s in (1, 120, 127, 134, 254):
        got = _native.mxfp4_to_float(*_block(list(range(16)) * 2, s))
        # the table read as float32: exact, but for the magnitudes 2 .. 6 under scale byte 254 -- beyond the largest float32: +-inf
        with np.errstate(over="ignore"):
            want = np.array([(-1.0 if c & 8 else 1.0) * MAGS[c & 7] * 2.0 ** (s - 127) for c in list(range(16)) * 2]).astype(np.float32)
        assert got.dtype == np.float32 and got.shape == (1, 32) and np.array_equal(got[0], want), s
    assert np.isnan(_native.mxfp4_to_float(*_block([0] * 32, 255))).all()


def test_to_mxfp4_round_trip_rounding_and_saturation():
    from hyperdb import _native
    rng = np.random.default_rng(3)
    # canonical blocks: the largest magnitude is 4 or 6 (so the shared exponent is the block's own), no negative zero
    codes = rng.integers(0, 16, size=(40, 96)).astype(np.uint8)
    codes[codes == 8] = 0
    codes[:, ::32] = rng.choice(np.array([6, 7, 14, 15], dtype=np.uint8), size=(40, 3))
    c = (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    s = rng.integers(1, 255, size=(40, 3)).astype(np.uint8)
    gc, gs = _native.to_mxfp4(_native.mxfp4_to_float(c, s))
    assert np.array_equal(gc, c) and np.array_equal(gs, s)
    # round to nearest even, by hand: amax = 4 keeps the exponent 0; ties go to the code with a clear mantissa bit
    x = np.zeros((1, 32))
    x[0, :12] = [4.0, 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, -2.5, 0.26, 0.24, 3.4, -0.75]
    gc, gs = _native.to_mxfp4(x)
    want = [4.0, 0.0, 1.0, 1.0, 2.0, 2.0, 4.0, -2.0, 0.5, 0.0, 3.0, -1.0]
    assert gs[0, 0] == 127 and np.array_equal(_native.mxfp4_to_float(gc, gs)[0, :12], np.array(want, dtype=np.float32))
    # saturation, by hand: amax = 7.5 has exponent 2, so the scale is 1 and 7.5, 7 and -6.5 saturate at +-6; 5 is a tie -> 4
    x[0, :5] = [7.5, 7.0, -6.5, 5.0, 5.1]
    gc, gs = _native.to_mxfp4(x[:, :32] * (np.arange(32) < 5))
    assert gs[0, 0] == 127 and np.array_equal(_native.mxfp4_to_float(gc, gs)[0, :5], np.array([6, 6, -6, 4, 6], dtype=np.float32))
    assert (_native.to_mxfp4(np.zeros((2, 64), dtype=np.float32))[1] == 127).all()
    for bad in (np.full((1, 32), np.nan), np.full((1, 32), np.inf), np.zeros((1, 48)), np.zeros(32)):
        with pytest.raises(ValueError, match="to_mxfp4"):
            _native.to_mxfp4(bad)


def test_rows_layout_and_input_policy():
    import torch
    from hyperdb import _native
    c = np.arange(5 * 192, dtype=np.uint8).reshape(5, 192)
    s = np.arange(5 * 12, dtype=np.uint8).reshape(5, 12) + 100
    rows = _native.pack_mxfp4_rows(c, s)
    assert rows.dtype == np.uint8 and rows.shape == (5, 208) == (5, _native.mxfp4_pitch(384))
    assert np.array_equal(rows[:, :192], c) and np.array_equal(rows[:, 192:204], s) and not rows[:, 204:].any()
    assert [_native.mxfp4_pitch(d) for d in (32, 384, 512, 1024)] == [32, 208, 272, 544]
    tc, ts = torch.from_numpy(c), torch.from_numpy(s)
    for pair in ((tc, ts), (tc.view(torch.float4_e2m1fn_x2), ts.view(torch.float8_e8m0fnu)), [c, s]):
        assert np.array_equal(_native.to_mxfp4_rows(pair, torch.device("cpu")).numpy(), rows)
    bad = (c, (c, s, s), (c.astype(np.float32), s), (c, s[:, :11]), (c[:, :8], s[:, :1]), (c[0], s[0]), (torch.zeros(5, 192), ts))
    for x in bad:
        with pytest.raises(ValueError, match="to_mxfp4"):
            _native.to_mxfp4_rows(x, torch.device("cpu"))
        with pytest.raises(ValueError, match="to_mxfp4"):
            _native.GpuIndex(x, storage="mxfp4")                   # (refused before a device is asked for)
    import hyperdb
    for make in (lambda: hyperdb.ranking_algorithm.register_vectors((c, s), devices=[0], storage="mxfp4"),
                 lambda: hyperdb.group.GpuGroup((c, s), [0], storage="mxfp4"), lambda: hyperdb.HyperDB(storage="mxfp4")):
        with pytest.raises(NotImplementedError, match="single index"):
            make()


def test_abi_version_dtype_width_and_alignment_checks():
    from hyperdb import _native
    lib = _native.lib()
    assert lib.hdb_version() >= 114
    h = ctypes.c_void_p()
    # dtype 13 passes the dtype check (the width check that FOLLOWS it refuses the row; no device is touched), 11 and 12 do not
    rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(16), 10, 100000 * 32, 13, 0, 0, None)
    assert rc == -1 and b"dtype" not in lib.hdb_last_error() and b"d too large" in lib.hdb_last_error()
    # unassigned codes; d no multiple of 32; a base that is not 16-byte aligned
    for ptr, d, dtype, msg in ((16, 64, 11, b"dtype"), (16, 64, 12, b"dtype"), (16, 64, 14, b"dtype"), (16, 48, 13, b"multiple of 32"),
                               (16, 33, 13, b"multiple of 32"), (24, 64, 13, b"16-byte aligned")):
        rc = lib.hdb_index_create(ctypes.byref(h), ctypes.c_void_p(ptr), 10, d, dtype, 0, 0, None)
        assert rc == -1 and msg in lib.hdb_last_error(), (ptr, d, dtype)
