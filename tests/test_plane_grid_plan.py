"""The grid of the plane pass (hdb_quant_plane_blocks and its table, csrc/hdb_caps.h) on the host.

tests/plane_grid_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, checks the rule over
n in {16, 17, 8193, 70001, 2 000 000, 10 000 000}, J = 1 .. 4, 1 / 64 / 256 CUs, plane_wg_per_cu = 0 .. 8 and max_blocks in {0, 1, 3, 5000}:
1 <= workgroups <= the cap, never more than the work, the max_blocks cap, the default equal to the table, no table entry above the
waves per SIMD its kernel is compiled for, and -- with hdb_plane_skip_* -- that the walk at every such grid still visits the complement
of the sample exactly once.  This file restates the rule in Python (plane_blocks; tests/test_plane_occupancy.py compares the stat
plane_blocks with it) and pins the restatement's table against the one the program prints.
No GPU call, nothing loaded into Python."""
import os
import re

import host_check
from host_check import CSRC


def wg_table():
    """HDB_PLANE_WG_PER_CU as the header states it: the default workgroups per CU for J = 1 .. 4"""
    text = open(os.path.join(CSRC, "hdb_caps.h")).read()
    m = re.search(r"^#define HDB_PLANE_WG_PER_CU \{(\d+), (\d+), (\d+), (\d+)\}$", text, re.M)
    assert m, "hdb_caps.h: HDB_PLANE_WG_PER_CU not found"
    return [int(x) for x in m.groups()]


def plane_blocks(nwalk, wg_per_cu, cus, max_blocks):
    """hdb_quant_plane_blocks with the workgroups per CU already chosen (1 .. 8)"""
    limit = wg_per_cu * max(cus, 1)
    if 0 < max_blocks < limit:
        limit = max_blocks
    return max(1, min(((nwalk + 1) // 2 + 3) // 4, limit))


def test_the_rule_and_the_walk_at_its_grids(tmp_path):
    out = host_check.run(host_check.build("plane_grid_check", tmp_path))
    assert "rules 2592\n" in out, "6 sizes, 4 widths, 3 devices, 9 settings of plane_wg_per_cu, 4 of max_blocks"
    table = [tuple(int(x) for x in line.split()[1:]) for line in out.splitlines() if line.startswith("table ")]
    assert [j for j, _, _ in table] == [1, 2, 3, 4] and [wg for _, wg, _ in table] == wg_table()
    for j, wg, waves in table:
        assert 1 <= wg <= waves <= 8, f"J = {j}: {wg} workgroups per CU, {waves} waves per SIMD compiled"
    walks = int(next(line.split()[1] for line in out.splitlines() if line.startswith("walks ")))
    assert walks >= 6 * 4 * 3, "every size and width is walked at several grids"
