"""The plans of an MXFP4 matrix wider than 512 elements under b1_mfma_min_q and f8_ks_min_q together (csrc/hdb_plan.h,
hdb_mfma_f4_wide_geom in csrc/hdb_caps.h): tests/mxf4_wide_plan_check.hip, a stand-alone host program under ASan / UBSan.  No GPU call."""
import host_check


def test_mxfp4_wide_row_plans(tmp_path):
    out = host_check.run(host_check.build("mxf4_wide_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    on = [int(line.split()[2]) for line in out.splitlines() if line.startswith("wide plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
    assert on and on[0] > 500, "the grid reaches the wide rows"
