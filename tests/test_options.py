"""The option table of csrc/hdb_plan.h (HDB_OPTIONS, hdb_option_set) on the host.

tests/golden/option_rules.jsonl was recorded from the strcmp ladder hdb_set_option had before the table: for every option name and
each of 28 values from -2^40 to 2^40 the member's value afterwards, starting from the defaults, and for the four options that
ignore a value outside their set one "valid, then invalid" pair.  tests/options_check.hip, a stand-alone host program with its own
main built under AddressSanitizer and UBSan, replays every line through hdb_option_set, and checks that each entry of the table
changes its own member's word of hdb_options and no other.  No line may be skipped: the program's line count is the file's.
No GPU call, nothing loaded into Python."""
import os

import host_check

RULES = os.path.join(host_check.GOLDEN, "option_rules.jsonl")


def test_option_table_keeps_the_recorded_rules(tmp_path):
    out = host_check.run(host_check.build("options_check", tmp_path), RULES)
    with open(RULES) as fh:
        lines = [line for line in fh if line.strip()]
    assert len(lines) > 1000 and f"lines {len(lines)}\n" in out, "the program replayed every line of the file"
