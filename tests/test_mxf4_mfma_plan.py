"""The plans of an MXFP4 matrix under the opt-in b1_mfma_min_q (csrc/hdb_plan.h, csrc/hdb_caps.h): tests/mxf4_mfma_plan_check.hip,
a stand-alone host program under ASan / UBSan.  No GPU call."""
import host_check


def test_mxfp4_matrix_core_plans(tmp_path):
    out = host_check.run(host_check.build("mxf4_mfma_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    on = [int(line.split()[2]) for line in out.splitlines() if line.startswith("mfma plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
    assert on and on[0] > 500, "the grid reaches the matrix cores"
