"""The K-slice lists of bfloat16 rows wider than 512 elements (ks_geom, csrc/hdb_caps.h) and the plans plan_topk (csrc/hdb_plan.h)
makes for them, on the host.

tests/bf16_wide_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only): every width of the bfloat16 slice table (640 .. 1536 in steps of 128, 2048, 3072, 4096) has slices of 256 / 384 / 512 elements
that add up to the row with cumulative byte offsets; the fp16 and float32 lists are the ones the uniform table gave; batches of 5+
dot / cosine / euclidean / pearson queries on a finite matrix plan the matrix cores through K slices (ld_ks = the rows rounded up
to 4, at most 128 queries per chunk, 16-row tiles), everything else keeps the VALU scan.  No GPU call, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")


def _hipcc():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert found, "hipcc not found (the library is built with it)"
    return found


def test_slice_lists_and_plans_of_wide_bf16_rows(tmp_path):
    exe = str(tmp_path / "bf16_wide_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "bf16_wide_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 10_000, "the program planned the whole grid"
