"""The host side of packed-bit storage (HDB_B1 = 10): the row pitch rule hdb_row_bytes (csrc/hdb_common.h), the capability rules
and the QT rule of the bit scan (csrc/hdb_caps.h), and the plans plan_topk (csrc/hdb_plan.h) makes for such a matrix.

tests/b1_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side only):
hdb_row_bytes is d * hdb_elem_bytes for every byte-sized dtype, d / 8 for packed bits at whole words and 0 otherwise; no
matrix-core, single-launch or tile-kernel rule admits the dtype; the tables of a pass fit the LDS the QT rule claims at every
admitted width; over the int8 check's grid every packed-bit plan keeps off the matrix cores, the shadow, the plane, the tile
kernel and the row list, equals the int8 plan for the bit metrics and the int8 plan with use_mfma = 0 for the others.
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


def test_packed_bit_pitch_rules_and_plans(tmp_path):
    exe = str(tmp_path / "b1_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "b1_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
