"""The K-slice lists of bfloat16 rows wider than 512 elements (ks_geom, csrc/hdb_caps.h) and the plans plan_topk (csrc/hdb_plan.h)
makes for them, on the host.

tests/bf16_wide_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only): every width of the bfloat16 slice table (640 .. 1536 in steps of 128, 2048, 3072, 4096) has slices of 256 / 384 / 512 elements
that add up to the row with cumulative byte offsets; the fp16 and float32 lists are the ones the uniform table gave; batches of 5+
dot / cosine / euclidean / pearson queries on a finite matrix plan the matrix cores through K slices (ld_ks = the rows rounded up
to 4, at most 128 queries per chunk, 16-row tiles), everything else keeps the VALU scan.  No GPU call, nothing loaded into Python."""

import host_check


def test_slice_lists_and_plans_of_wide_bf16_rows(tmp_path):
    out = host_check.run(host_check.build("bf16_wide_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 10_000, "the program planned the whole grid"
