"""The two stages of the plane pass (hdb_plane_rho4, hdb_plane_r4_up, hdb_plane_interval, hdb_plane_div_u, csrc/hdb_caps.h) on the host.

tests/plane_bit_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, packs code rows the way
the plane is derived and decodes them with the masks of the two stages: c = 16 n - 120 + rho4 for every code, 2 S4 + S1 the five-bit
sum, ch4 >= fl(C) >= cl4 with R4 from the row's own rho4 for every U (random and extreme rows and queries), a tile's R4* at or above
every row's, and the division-free slot number of stage B.
No GPU call, nothing loaded into Python."""

import host_check


def test_stages(tmp_path):
    out = host_check.run(host_check.build("plane_bit_check", tmp_path))
    assert "codes 255\n" in out, "every code -127 .. 127"
    assert "rows 4608\n" in out, "16 rows x 6 queries x 3 widths for each of U = 1 .. 16"
    assert "tiles 288\n" in out
    assert "divisions 4352\n" in out, "every idx < 32 U, U = 1 .. 16"
