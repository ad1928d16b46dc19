"""plan_topk (csrc/hdb_plan.h), the one place hdb_topk chooses its path, replayed on the host; and the live library against the
same table.

tests/golden/dispatch_table.jsonl was recorded by tools/dispatch_table.py from the library BEFORE the planner existed: one hdb_topk
call per line, its inputs and the statistics that library defined on the call's path.
  * test_plan_reproduces_the_table: tests/topk_plan_check.hip, a stand-alone host program with its own main built under
    AddressSanitizer and UBSan, feeds every row's facts to plan_topk and compares the plan's statistics field by field, then checks
    the plan's properties on every row and over a synthetic grid (nq x n x d x dtype x metric x k x status x exact x finiteness).
    No GPU call, nothing loaded into Python.  No row may be skipped: the program's row count is the file's.
  * test_live_library_matches_the_table (GPU): the rows of up to 70 001 stored rows, run again on the built library."""
import json
import os
import sys

import pytest

import host_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "dispatch_table.jsonl")


def _table():
    with open(TABLE) as fh:
        return [json.loads(line) for line in fh if line.strip()]


def test_plan_reproduces_the_table(tmp_path):
    out = host_check.run(host_check.build("topk_plan_check", tmp_path), TABLE)
    lines = _table()
    assert "header" in lines[0] and lines[0]["rows"] == len(lines) - 1
    assert f"rows {len(lines) - 1}\n" in out, "the program read every row of the table"


@pytest.mark.gpu
def test_live_library_matches_the_table():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_table
    want = [row for row in _table()[1:] if int(row["call"].split()[2]) <= 70001]
    got = dispatch_table.record(max_n=70001)[1:]
    assert len(got) == len(want) and len(want) > 100
    key = lambda row: json.dumps({k: v for k, v in row.items() if k != "stats"}, sort_keys=True)
    want_by = {}
    for row in want:
        want_by.setdefault(key(row), []).append(row)
    for row in got:                        # (the tool runs its rows group by group: match them by their inputs, in order)
        assert want_by.get(key(row)), f"a call the table does not hold: {row}"
        assert row == want_by[key(row)].pop(0)
