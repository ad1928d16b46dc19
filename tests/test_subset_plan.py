"""The row-list rule of plan_topk (csrc/hdb_plan.h) on the host: tests/subset_plan_check.hip, a stand-alone program with its own main
built under AddressSanitizer and UBSan, takes hdb_plan.h only.  Over dtype x d x n x m x nq x k x metric x exact it checks that a plan
that takes the list is the multi-kernel pipeline with the extents and statistics of the same call on a matrix of m rows (matrix cores,
single launches, shadow and tile kernel off), that the bit metrics, use_subset = 0, an empty list, a violated ratio rule, a matrix
below subset_min_n and a full sort inside never take it and are the masked plan field by field, and that every row of the recorded
dispatch table (tests/golden/dispatch_table.jsonl) plans as before.  No GPU call, nothing loaded into Python."""
import json
import os

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "dispatch_table.jsonl")


def test_subset_plan(tmp_path):
    out = host_check.run(host_check.build("subset_plan_check", tmp_path), TABLE)
    with open(TABLE) as fh:
        lines = [json.loads(line) for line in fh if line.strip()]
    assert f"rows {len(lines) - 1}\n" in out, "the program read every row of the table"
