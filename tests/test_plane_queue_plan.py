"""The pending queue between the two stages of the plane pass (hdb_plane_vt_map, HdbPlanePending, csrc/hdb_caps.h) on the host.

tests/plane_queue_check.hip, a stand-alone program with its own main built under AddressSanitizer and UBSan, checks the virtual-tile
map of stage B (slot = idx / U, unit = idx % U, word = row U + unit, against plain division, for every U = 1 .. 16 and every piece a
lane can hold) and runs a model of the two wave-private queues over random, all-kept, none-kept and ragged step sequences: never more
than 48 entries in either, every pending entry flushed exactly once, every survivor drained exactly once.
No GPU call, nothing loaded into Python."""

import host_check


def test_queue(tmp_path):
    out = host_check.run(host_check.build("plane_queue_check", tmp_path))
    assert "maps 2560\n" in out, "every f < 64 J, U = 1 .. 16: 64 x (4 x 1 + 4 x 2 + 4 x 3 + 4 x 4)"
    lines = dict(line.split() for line in out.splitlines() if line and line.split()[0] in ("steps", "entries", "survivors"))
    assert int(lines["steps"]) >= 64 * 200 + 100
    assert int(lines["entries"]) > 0 and 0 < int(lines["survivors"]) < int(lines["entries"])
