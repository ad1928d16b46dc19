"""The stand-alone host check programs (tests/NAME.hip, each with its own main): built with hipcc under AddressSanitizer and UBSan --
host side only -- and run as a child process.  No GPU call, nothing loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "local-hyperdb_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def build(name, tmp_path):
    """Compile tests/NAME.hip into tmp_path -> the program's path."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    found = hipcc if os.path.exists(hipcc) else shutil.which("hipcc")
    assert found, "hipcc not found (the library is built with it)"
    exe = str(tmp_path / name)
    done = subprocess.run([found, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                           os.path.join(ROOT, "tests", name + ".hip"), "-o", exe],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    return exe


def run(exe, *args):
    """Run the program: exit status 0, " 0 failures", nothing from a sanitizer -> its standard output."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    done = subprocess.run([exe, *args], capture_output=True, text=True, env=env)
    print(done.stdout)
    assert done.returncode == 0, done.stdout + done.stderr
    assert " 0 failures" in done.stdout and "runtime error" not in done.stderr and "AddressSanitizer" not in done.stderr
    return done.stdout
