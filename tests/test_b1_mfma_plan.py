"""The plans of a packed-bit matrix under the opt-in b1_mfma_min_q (csrc/hdb_plan.h) and the rules beside it (csrc/hdb_caps.h).

tests/b1_mfma_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only): the whole widths and the slice lists of the packed-bit matrix-core kernels; with the option at 0 every plan is today's; with
it on, a packed-bit plan equals the int8 plan (whole rows) or the float8 K-slice plan (wider rows) made with the threshold in force,
and today's plan wherever the bit scan keeps the call; the finiteness callback is never asked.
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


def test_packed_bit_matrix_core_plans(tmp_path):
    exe = str(tmp_path / "b1_mfma_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "b1_mfma_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    on = [int(line.split()[2]) for line in run.stdout.splitlines() if line.startswith("mfma plans ")]
    assert plans and plans[0] > 1_000_000, "the program planned the whole grid"
    assert on and on[0] > 10_000, "the grid reaches the matrix cores"
