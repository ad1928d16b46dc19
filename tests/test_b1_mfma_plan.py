"""The plans of a packed-bit matrix under the opt-in b1_mfma_min_q (csrc/hdb_plan.h) and the rules beside it (csrc/hdb_caps.h).

tests/b1_mfma_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only): the whole widths and the slice lists of the packed-bit matrix-core kernels; with the option at 0 every plan is today's; with
it on, a packed-bit plan equals the int8 plan (whole rows) or the float8 K-slice plan (wider rows) made with the threshold in force,
and today's plan wherever the bit scan keeps the call; the finiteness callback is never asked.
No GPU call, nothing loaded into Python."""

import host_check


def test_packed_bit_matrix_core_plans(tmp_path):
    out = host_check.run(host_check.build("b1_mfma_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    on = [int(line.split()[2]) for line in out.splitlines() if line.startswith("mfma plans ")]
    assert plans and plans[0] > 1_000_000, "the program planned the whole grid"
    assert on and on[0] > 10_000, "the grid reaches the matrix cores"
