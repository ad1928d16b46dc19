"""The host side of float8 e4m3 storage (HDB_F8E4M3 = 5): the exact widening helper, the capability rules (csrc/hdb_caps.h) and
the plans plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/f8_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
each of the 256 codes widens to the value its fields spell; no width has a matrix-core geometry, a single launch or the LDS tile
kernel; the VALU scan's grid grows for 256- / 384- / 512-byte rows only; over a grid of n, d, nq, k, metric and option values no
plan uses the shadow, the plane, a matrix-core single launch or the matrix cores, and every plan equals the plan of a bfloat16
matrix of the same shape with the matrix cores off (small, sampled, exact, full sort, row list), with 16-row sample tiles.
No GPU call, nothing loaded into Python."""
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


def test_float8_widening_rules_and_plans(tmp_path):
    exe = str(tmp_path / "f8_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "f8_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
