"""The plans of an MXFP4 matrix under f8_lds_min_q beside b1_mfma_min_q (csrc/hdb_plan.h, the hdb_mfma_f4_lds_* rules of
csrc/hdb_caps.h): tests/mxf4_lds_plan_check.hip, a stand-alone host program under ASan / UBSan.  No GPU call."""
import host_check


def test_mxfp4_lds_flavour_plans(tmp_path):
    out = host_check.run(host_check.build("mxf4_lds_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    on = [int(line.split()[2]) for line in out.splitlines() if line.startswith("lds plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
    assert on and on[0] > 500, "the grid reaches the LDS flavour"
