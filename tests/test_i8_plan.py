"""The host side of int8 storage (HDB_I8 = 7): the exact widening helpers, the capability rules (csrc/hdb_caps.h) and the plans
plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/i8_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
each of the 256 codes widens to its integer and the upper 16 bits of that float32 carry the whole value; the capability rules
answer for int8 what they answer for float8; over the float8 check's grid of n, d, nq, k, metric and option values every int8
plan equals the float8 plan with the two float8 opt-ins (K slices, LDS flavour) at 0.  No GPU call, nothing loaded into Python."""

import host_check


def test_int8_widening_rules_and_plans(tmp_path):
    out = host_check.run(host_check.build("i8_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
