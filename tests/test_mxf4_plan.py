"""The host side of MXFP4 storage (HDB_MXF4 = 13): pitches and plans, tests/mxf4_plan_check.hip under ASan / UBSan.  No GPU call."""
import host_check


def test_mxfp4_pitch_rules_and_plans(tmp_path):
    out = host_check.run(host_check.build("mxf4_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
