"""The opt-in int8 shadow of a bfloat16 index on the host: the plans plan_topk (csrc/hdb_plan.h) makes for bfloat16 facts.

tests/bf16_quant_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only).  Grid A: a bfloat16 index that holds an explicit shadow takes HDB_PATH_QUANT (VALU flavour, nothing to build, quant = 1,
mfma = 0) exactly for 1-4 dot / cosine / euclidean queries, k <= 128, status words, not exact, a finite matrix above HDB_CAND_CAP
rows and the row rule (quant_min_rows(HDB_BF16) or quant_min_n); plane_wanted exactly for one dot / cosine query, d <= 512, at the
plane's row rule; the finiteness is asked at most once; use_quant = 0 takes nothing.  Grid B: a bfloat16 index without a shadow
never plans one and never asks for a build, under default options and under quant_min_n = 0, and its plan equals the plan with the
shadow rules switched off.  No GPU call, nothing loaded into Python."""
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


def test_plans_of_bf16_facts_with_and_without_a_shadow(tmp_path):
    exe = str(tmp_path / "bf16_quant_plan_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "bf16_quant_plan_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    plans = [int(line.split()[1]) for line in run.stdout.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
