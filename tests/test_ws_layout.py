"""The workspace layouts of csrc/hdb_ws.h, run on the host under AddressSanitizer and UBSan.

Each workspace of hdb_api.hip is laid out by ONE function that both sizes it (a Bump without a base) and places its pointers.
tests/ws_layout_check.hip, a stand-alone program with its own main, runs the four layouts over
    nq in {1, 4, 5, 256, 300} x n in {1, 8192, 8193, 70001, 10^7} x d in {1, 40, 384, 4096} x k in {1, 128, 2049}
and every flag combination they take (exact, small, K slices, full sort, matrix-core flavour, plane).  The program states the bytes
needed behind every pointer of a layout and checks at each point that every region is 256-byte aligned and holds those bytes, that
regions do not overlap and lie inside the reported size, and that no layout needs more bytes than the byte formula it replaced.
Shadow layouts and k: QuantWs::lay takes no k by construction; what the program checks is that the plan it is sized with
(quant_ld_max, hdb_ws.h -- the one hdb_api.hip uses) holds the sample of k = 1, 128 and 2049, so the size is the same for each.
That a live index keeps its workspace over k is tests/test_workspace_reuse.py's part.  No GPU is used."""

import host_check


def test_layouts_over_the_grid(tmp_path):
    out = host_check.run(host_check.build("ws_layout_check", tmp_path))
