"""The host side of the LDS flavour of the float8 matrix-core scan (csrc/hdb_mfma_f8_lds.h): its geometry (csrc/hdb_caps.h) and the
plans plan_topk (csrc/hdb_plan.h) makes under the option f8_lds_min_q.

tests/f8_lds_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
for every supported width and 4 / 8 waves the stage is a multiple of 16 rows and both buffers fit 160 KiB; with f8_lds_min_q = 0 no
plan takes the flavour; with n or -1 a plan takes it exactly where it is on the float8 matrix cores (whole rows of 128 .. 512
elements, or K slices under f8_ks_min_q) outside the full sort with max(n, 5, mfma_min_q) queries -- never for another dtype, small
matrices, row-list calls, matrices that are not finite or manhattan; and every other field of every plan equals the plan with the
option off.  No GPU call, nothing loaded into Python."""

import host_check


def test_lds_flavour_geometry_and_plans(tmp_path):
    out = host_check.run(host_check.build("f8_lds_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
