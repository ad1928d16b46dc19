"""The host side of packed-bit storage (HDB_B1 = 10): the row pitch rule hdb_row_bytes (csrc/hdb_common.h), the capability rules
and the QT rule of the bit scan (csrc/hdb_caps.h), and the plans plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/b1_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
hdb_row_bytes is d * hdb_elem_bytes for every byte-sized dtype, d / 8 for packed bits at whole words and 0 otherwise; no
matrix-core, single-launch or tile-kernel rule admits the dtype; the tables of a pass fit the LDS the QT rule claims at every
admitted width; over the int8 check's grid every packed-bit plan keeps off the matrix cores, the shadow, the plane, the tile
kernel and the row list, equals the int8 plan for the bit metrics and the int8 plan with use_mfma = 0 for the others.
No GPU call, nothing loaded into Python."""

import host_check


def test_packed_bit_pitch_rules_and_plans(tmp_path):
    out = host_check.run(host_check.build("b1_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
