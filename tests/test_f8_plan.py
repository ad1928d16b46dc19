"""The host side of float8 e4m3 storage (HDB_F8E4M3 = 5): the exact widening helper, the capability rules (csrc/hdb_caps.h) and
the plans plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/f8_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
each of the 256 codes widens to the value its fields spell; no width has a matrix-core geometry, a single launch or the LDS tile
kernel; the VALU scan's grid grows for 256- / 384- / 512-byte rows only; over a grid of n, d, nq, k, metric and option values no
plan uses the shadow, the plane, a matrix-core single launch or the matrix cores, and every plan equals the plan of a bfloat16
matrix of the same shape with the matrix cores off (small, sampled, exact, full sort, row list), with 16-row sample tiles.
No GPU call, nothing loaded into Python."""

import host_check


def test_float8_widening_rules_and_plans(tmp_path):
    out = host_check.run(host_check.build("f8_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
