"""The opt-in K slices of float8 e4m3 rows wider than 512 elements on the host: the slice lists (ks_geom_f8, csrc/hdb_caps.h) and
the plans plan_topk (csrc/hdb_plan.h) makes under the option f8_ks_min_q.

tests/f8_wide_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only): ks_geom_f8 has slices exactly at bfloat16's widths, equal to ks_geom_bf16's slice by slice, with cumulative element offsets
that are multiples of 8; the caps of the default dispatch (hdb_mfma_ksplit_slices, hdb_mfma_tile_rows, hdb_mfma_supported) stay 0
for float8 beyond 512 elements; with default options no float8 plan takes the slices; with f8_ks_min_q = 5 the slices are planned
exactly for 5+ dot / cosine / euclidean / pearson queries on a finite matrix of a sliced width, as the bfloat16 plan of the same
shape; 9 starts at 9 queries, -1 follows hdb_mfma_f8_ks_min_q, 3 is clamped to 5.  No GPU call, nothing loaded into Python."""

import host_check


def test_slice_lists_and_plans_of_wide_f8_rows(tmp_path):
    out = host_check.run(host_check.build("f8_wide_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 10_000, "the program planned the whole grid"
