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
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "dispatch_table.jsonl")


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert found, "hipcc not found (the library is built with it)"
    return found


def _table():
    with open(TABLE) as fh:
        return [json.loads(line) for line in fh if line.strip()]


def test_plan_reproduces_the_table(tmp_path):
    exe = str(tmp_path / "topk_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "topk_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, TABLE], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    lines = _table()
    assert "header" in lines[0] and lines[0]["rows"] == len(lines) - 1
    assert f"rows {len(lines) - 1}\n" in run.stdout, "the program read every row of the table"


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
