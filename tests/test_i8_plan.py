"""The host side of int8 storage (HDB_I8 = 7): the exact widening helpers, the capability rules (csrc/hdb_caps.h) and the plans
plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/i8_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
each of the 256 codes widens to its integer and the upper 16 bits of that float32 carry the whole value; the capability rules
answer for int8 what they answer for float8; over the float8 check's grid of n, d, nq, k, metric and option values every int8
plan equals the float8 plan with the two float8 opt-ins (K slices, LDS flavour) at 0.  No GPU call, nothing loaded into Python."""
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


def test_int8_widening_rules_and_plans(tmp_path):
    exe = str(tmp_path / "i8_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "i8_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
