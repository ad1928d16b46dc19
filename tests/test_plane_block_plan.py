"""The hot block of the plane pass (hdb_plane_k_*, hdb_plane_rc_*, hdb_plane_block_off, csrc/hdb_caps.h) on the host.

tests/plane_block_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, runs the very functions
the two kernels use: the outward bfloat16 rounding of a row's scale over every finite non-negative bfloat16 pattern and its float32
and float64 neighbours (k_hi >= k >= k_lo, k_hi the smallest), the byte code of the residual norm over every integer sum of squares
up to 16 x 512 (0.5 rc >= sqrt(ss), rc the smallest, at most 182), and the block offsets (two 64-byte blocks and 128 reserved bytes
tile the 256 bytes of a tile's records, U = 1 .. 16).
No GPU call, nothing loaded into Python."""

import host_check


def test_codes_and_offsets(tmp_path):
    out = host_check.run(host_check.build("plane_block_check", tmp_path))
    assert "patterns 32640\n" in out, "every finite non-negative bfloat16: 0x0000 .. 0x7F7F"
    assert "sums 8193\n" in out, "every integer sum of squared residuals up to 16 x 512"
    assert "tiles 656\n" in out, "41 tiles for each of U = 1 .. 16"
