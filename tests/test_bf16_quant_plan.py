"""The opt-in int8 shadow of a bfloat16 index on the host: the plans plan_topk (csrc/hdb_plan.h) makes for bfloat16 facts.

tests/bf16_quant_plan_check.hip is a stand-alone host program with its own main, built under AddressSanitizer and UBSan (host side
only).  Grid A: a bfloat16 index that holds an explicit shadow takes HDB_PATH_QUANT (VALU flavour, nothing to build, quant = 1,
mfma = 0) exactly for 1-4 dot / cosine / euclidean queries, k <= 128, status words, not exact, a finite matrix above HDB_CAND_CAP
rows and the row rule (quant_min_rows(HDB_BF16) or quant_min_n); plane_wanted exactly for one dot / cosine query, d <= 512, at the
plane's row rule; the finiteness is asked at most once; use_quant = 0 takes nothing.  Grid B: a bfloat16 index without a shadow
never plans one and never asks for a build, under default options and under quant_min_n = 0, and its plan equals the plan with the
shadow rules switched off.  No GPU call, nothing loaded into Python."""

import host_check


def test_plans_of_bf16_facts_with_and_without_a_shadow(tmp_path):
    out = host_check.run(host_check.build("bf16_quant_plan_check", tmp_path))
    plans = [int(line.split()[1]) for line in out.splitlines() if line.startswith("plans ")]
    assert plans and plans[0] > 100_000, "the program planned the whole grid"
