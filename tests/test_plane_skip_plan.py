"""The walk of the plane pass over the tiles the sample pass did not take (hdb_plane_skip_*, csrc/hdb_caps.h) on the host.

tests/plane_skip_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, walks the tiles exactly as
hdb_quant_plane_scan_kernel does -- start (block * 4 + wave) * 2, step grid * 8, one division where the walk starts and incremental
updates after it -- for n in {16, 17, 8193, 8217, 70001, 1 000 003, 10 000 000} with the call's own sample, forced plans (stride 1 among
them) and grids of 1, 3 and 1024 workgroups, and checks that the visited tiles are the complement of the sampled ones, each exactly
once, and that every sampled tile is hdb_tile_index(w, stride).  It also prints hdb_tile_index for a fixed list of (w, stride): this
file compares them with tile_index below, the Python restatement tests/test_plane_skip.py plants its rows with.
No GPU call, nothing loaded into Python."""

import host_check


def tile_index(t, stride):
    """hdb_tile_index (csrc/hdb_common.h): sample tile t of a strided sample sits at t * stride + a fixed jitter below stride"""
    if stride == 1:
        return t
    h = (t * 2654435761) & 0xFFFFFFFF
    return t * stride + (h >> 8) % stride


def test_walk_is_the_complement_of_the_sample(tmp_path):
    out = host_check.run(host_check.build("plane_skip_check", tmp_path))
    assert "plans 51\n" in out, "7 sizes and 10 forced plans, three grids each"
    pinned = [tuple(int(x) for x in line.split()[1:]) for line in out.splitlines() if line.startswith("index ")]
    assert len(pinned) == 63
    for w, stride, value in pinned:
        assert tile_index(w, stride) == value, f"tile_index({w}, {stride}) = {tile_index(w, stride)}, the library says {value}"
    assert any(value != w * stride for w, stride, value in pinned if stride > 1), "the jitter is exercised"
