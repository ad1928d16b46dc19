"""The numpy model of the selection contract (tests/select_model.py) against a brute-force Python sort, and the coverage of its
case tables: every branch label of hdb_finalize_fast / hdb_finalize_body at 256, 512 and 1024 threads.  No GPU."""
import os
import struct

import numpy as np
import pytest

import select_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def _brute_topk(scores, k, row_base):
    """Python floats compare as float32 values do (the arrays are canonical: no NaN, no -0.0)."""
    t = sorted((-float(s), r) for r, s in enumerate(scores))
    idx = [r + row_base for _, r in t[:k]] + [-1] * max(k - len(t), 0)
    bits = [_bits(-ns) for ns, _ in t[:k]] + [0xFF800000] * max(k - len(t), 0)
    return idx, bits


SMALL_N = (1, 2, 7, 63, 300)


@pytest.mark.parametrize("n", SMALL_N)
def test_topk_equals_a_brute_force_sort_on_every_family(n):
    for k in (1, 2, 17, 64, 400):
        specs = sm._family_specs(n, k)
        assert {s[0] for s in specs} == set(sm.FAMILIES)
        for i, spec in enumerate(specs):
            s = sm.make_scores(spec, n, 11 + i)
            assert not np.isnan(s).any() and not (np.signbit(s) & (s == 0)).any(), sm.spec_name(spec)
            for row_base in (0, 2 ** 33 + 5):
                idx, bits = sm.topk(s, n, k, row_base)
                bi, bb = _brute_topk(s, k, row_base)
                assert idx.dtype == np.int64 and bits.dtype == np.uint32
                assert idx.tolist() == bi and bits.tolist() == bb, (sm.spec_name(spec), n, k)


@pytest.mark.parametrize("n", SMALL_N)
def test_finalize_equals_a_brute_force_sort_on_every_family(n):
    rng = np.random.default_rng(n)
    for k, kk in ((1, 1), (5, 3), (64, 64), (400, 350)):
        for i, spec in enumerate(sm._family_specs(n, k)):
            s = sm.make_scores(spec, n, 23 + i)
            rows = rng.permutation(5 * n)[:n]
            entries = sm.pack(s, rows)
            for total, cap, qnan, inf_status in ((n, 8192, 0, 0), (n + 9, n, 3, 1), (n, max(n - 1, 1), 2, 0), (n, 8192, 1, 1)):
                nc = min(total, cap)
                idx, bits, st = sm.finalize(entries, total, cap, k, kk, 100, qnan, inf_status)
                t = sorted((-float(s[j]), int(rows[j])) for j in range(nc))
                nout = min(nc, kk)
                assert idx.tolist() == [r + 100 for _, r in t[:nout]] + [-1] * (k - nout), (sm.spec_name(spec), n, k)
                assert bits.tolist() == [_bits(-ns) for ns, _ in t[:nout]] + [0xFF800000] * (k - nout)
                want = (sm.Q_OVERFLOW if total > cap else 0) | (sm.Q_UNDERFLOW if nc < kk else 0) | (sm.Q_NAN if qnan & 1 else 0) | \
                       (inf_status if qnan & 2 else 0)
                assert st == want


def test_keys_are_strictly_monotone_and_round_trip():
    classes = [-np.inf, -3.4028235e38, -1e30, -2.0, -1.0000001, -1.0, -0.99999994, -1.1754944e-38, -1.1754942e-38, -1e-45, 0.0, 1e-45,
               1.1754942e-38, 1.1754944e-38, 0.99999994, 1.0, 1.0000001, 2.0, 1e30, 3.4028235e38, np.inf]
    rng = np.random.default_rng(0)
    rnd = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    rnd = rnd[~np.isnan(rnd)]
    x = np.unique(sm.canon(np.concatenate([np.array(classes, dtype=np.float32), rnd])))      # sorted ascending, distinct values
    keys = sm.f2key(x)
    assert (np.diff(keys.astype(np.int64)) > 0).all()
    assert keys.min() > 0                                   # key 0 is below every real score, -inf included
    assert (sm.fbits(sm.key2f(keys)) == sm.fbits(x)).all()
    # -0.0 and NaN are not canonical, but the bijection holds for every bit pattern
    allbits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    assert (sm.fbits(sm.key2f(sm.f2key(allbits.view(np.float32)))) == allbits).all()
    assert int(sm.pack(np.float32(1.0), 5).reshape(-1)[0]) == ((0xBF800000 << 32) | (0xFFFFFFFF - 5))


def test_byte0_ulp_chain_is_a_nextafter_chain():
    for centre, away in ((1.0, np.inf), (-1.0, -np.inf)):
        s = np.unique(sm.ulp_chain(256, 0, centre=centre, byte=0))
        s = s if centre > 0 else s[::-1]
        assert len(s) == 256 and s[0] == np.float32(centre)
        assert (np.nextafter(s[:-1], np.float32(away)) == s[1:]).all()
    for byte in (1, 2):
        k = sm.f2key(sm.ulp_chain(1000, 0, centre=-1.0, byte=byte))
        assert len(np.unique(k)) == 256 and len(np.unique(k & ~np.uint32(0xFF << (8 * byte)))) == 1


def test_sample_threshold_is_a_lower_bound_of_the_mth_largest():
    for n in sm.SAMPLE_N:
        for m in sm.SAMPLE_M:
            for i, spec in enumerate(sm.THRESHOLD_SPECS):
                s = sm.make_scores(spec, n, i)
                thr = np.array([sm.sample_threshold(s, n, m)], dtype=np.uint32).view(np.float32)[0]
                if n < m:
                    assert thr == -np.inf
                else:
                    assert thr <= sm.mth_largest_bits(s, n, m)
                if n >= m and n <= 4 * 1024 and m == 1:
                    assert thr == s.max()                      # one maximum: always found


def test_branch_labels_cover_every_branch_at_every_thread_count():
    seen = {t: set() for t in sm.THREADS}
    for c in sm.finalize_cases():
        lab = sm.finalize_case_labels(c)
        assert lab <= set(sm.LABELS)
        seen[c["threads"]] |= lab
        built = sm.LAYOUT_BUILT_FOR.get(c["layout"])
        if built and 256 < c["nc"] <= 16 * c["threads"] and 16 <= c["kk"] <= 256 and c["total"] == c["nc"]:
            assert built <= lab, (c, sorted(lab))
        if c["layout"] == "ties300" and c["threads"] == 256 and "fast" in lab:
            assert "fallback_ns_gt_threads" in lab and "fallback_ns_gt_1024" not in lab, (c, sorted(lab))
    for t in sm.THREADS:
        assert seen[t] == set(sm.LABELS), (t, sorted(set(sm.LABELS) - seen[t]))


def test_case_tables_hold_the_sizes_the_kernels_switch_at():
    ex = sm.exact_cases()
    assert {c["n"] for c in ex} == set(sm.EXACT_N) and {c["k"] for c in ex} >= set(sm.EXACT_K)
    assert {s[0] for c in ex for s in c["specs"]} == set(sm.FAMILIES)
    assert {s[2] for c in ex for s in c["specs"]} == {None, "asc", "desc", "shuf"}
    assert all(3 <= len(c["specs"]) <= 4 for c in ex)
    assert any(c["row_base"] == 2 ** 33 + 5 for c in ex)
    assert {(d, c["npass"]) for c in ex for s in c["specs"] if s[0] == "int_levels" and c["npass"] < 4 for d in [s[1]["d"]]} == \
        {(8, 2), (40, 2), (384, 3)}
    assert all(s[0] in ("int_levels", "one_level") for c in ex if c["npass"] < 4 for s in c["specs"])
    fin = sm.finalize_cases()
    assert {c["nc"] for c in fin} >= set(sm.FIN_NC) and {c["threads"] for c in fin} == set(sm.THREADS)
    assert {c["total"] for c in fin if c["total"] != c["nc"]} == {sm.CAP + 5}
    assert {(c["qnan"], c["inf_status"]) for c in fin} == {(q, s) for q in range(4) for s in (0, sm.Q_UNDERFLOW)}
    assert any(c["kk"] > c["nc"] for c in fin)
    for nc in sm.FIN_NC:
        kks = {c["kk"] for c in fin if c["nc"] == nc}
        assert kks >= {1, 16, 255, 256, 257, 2048}
        if nc >= 4:
            assert kks >= {nc // 2 - 1, nc // 2}
    caps = [sm.collect_counts(sm.make_scores(c["spec"], c["n"], 3), c["n"], c["k"]) for c in sm.capacity_cases()]
    assert {(cnt, ti[2], ti[3]) for cnt, ti in caps} == {(sm.CAP, 1, 100), (200, 0, 100)}


def test_coverage_table_is_current():
    with open(os.path.join(ROOT, "profiles", "select_coverage.txt")) as f:
        assert f.read() == sm.coverage_text(), "regenerate with: python tests/select_model.py"
