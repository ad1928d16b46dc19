"""The hot block of the plane pass (hdb_plane_k_*, hdb_plane_rc_*, hdb_plane_block_off, csrc/hdb_caps.h) on the host.

tests/plane_block_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, runs the very functions
the two kernels use: the outward bfloat16 rounding of a row's scale over every finite non-negative bfloat16 pattern and its float32
and float64 neighbours (k_hi >= k >= k_lo, k_hi the smallest), the byte code of the residual norm over every integer sum of squares
up to 16 x 512 (0.5 rc >= sqrt(ss), rc the smallest, at most 182), and the block offsets (two 64-byte blocks and 128 reserved bytes
tile the 256 bytes of a tile's records, U = 1 .. 16).
No GPU call, nothing loaded into Python."""
import os
import subprocess

from test_plane_skip_plan import CSRC, ROOT, _hipcc


def test_codes_and_offsets(tmp_path):
    exe = str(tmp_path / "plane_block_check")
    build = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", "-I", CSRC,
                            os.path.join(ROOT, "tests", "plane_block_check.hip"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr
    assert "patterns 32640\n" in run.stdout, "every finite non-negative bfloat16: 0x0000 .. 0x7F7F"
    assert "sums 8193\n" in run.stdout, "every integer sum of squared residuals up to 16 x 512"
    assert "tiles 656\n" in run.stdout, "41 tiles for each of U = 1 .. 16"
