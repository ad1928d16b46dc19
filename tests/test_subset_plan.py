"""The row-list rule of plan_topk (csrc/hdb_plan.h) on the host: tests/subset_plan_check.hip, a stand-alone program with its own main
built under AddressSanitizer and UBSan, takes hdb_plan.h only.  Over dtype x d x n x m x nq x k x metric x exact it checks that a plan
that takes the list is the multi-kernel pipeline with the extents and statistics of the same call on a matrix of m rows (matrix cores,
single launches, shadow and tile kernel off), that the bit metrics, use_subset = 0, an empty list, a violated ratio rule, a matrix
below subset_min_n and a full sort inside never take it and are the masked plan field by field, and that every row of the recorded
dispatch table (tests/golden/dispatch_table.jsonl) plans as before.  No GPU call, nothing loaded into Python."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")
TABLE = os.path.join(ROOT, "tests", "golden", "dispatch_table.jsonl")


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert found, "hipcc not found (the library is built with it)"
    return found


def test_subset_plan(tmp_path):
    exe = str(tmp_path / "subset_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "subset_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe, TABLE], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    with open(TABLE) as fh:
        lines = [json.loads(line) for line in fh if line.strip()]
    assert f"rows {len(lines) - 1}\n" in run.stdout, "the program read every row of the table"
