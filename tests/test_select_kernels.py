"""The top-k selection kernels (hdb_select.hip, hdb_finalize.h) against the numpy model of tests/select_model.py, driven directly
through their launchers (tests/select_harness.py) with score arrays and candidate lists built to steer every data-dependent
branch: crowded bins, lists straddling zero, ties beyond the survivor list / the workgroup / the candidate capacity, consecutive
ulps, denormals, +-inf as scores, padded rows with live values behind n, and finalize at 256, 512 and 1024 threads.

Every comparison is bit-exact: indices, float32 score bits, status words, counters, tie_info, thresholds."""
import numpy as np
import pytest

import select_model as sm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hx():
    import torch
    assert torch.cuda.is_available(), "the selection kernel tests need the GPU"
    import select_harness
    for name in select_harness._SIGNATURES:
        select_harness.fn(name)                 # a missing export fails here
    return select_harness


def _check_query(tag, got_idx, got_bits, want_idx, want_bits):
    if (got_idx != want_idx).any() or (got_bits != want_bits).any():
        bad = np.flatnonzero((got_idx != want_idx) | (got_bits != want_bits))
        j = int(bad[0])
        raise AssertionError("%s: %d of %d slots differ, first at %d: got (%d, %#010x) want (%d, %#010x)" % (
            tag, len(bad), len(want_idx), j, got_idx[j], got_bits[j], want_idx[j], want_bits[j]))


# ---- exact selection: hist x npass, collect, finalize ----------------------------------------------------------------------
@pytest.mark.parametrize("n", sm.EXACT_N)
def test_exact_selection_equals_the_model(hx, n):
    cases = [c for c in sm.exact_cases() if c["n"] == n]
    assert cases
    for c in cases:
        k, kk = c["k"], min(c["k"], n)
        arrays = [sm.make_scores(spec, n, c["seed"] + qi) for qi, spec in enumerate(c["specs"])]
        r = hx.exact_select(arrays, n, k, c["npass"], c["row_base"])
        for qi, (spec, s) in enumerate(zip(c["specs"], arrays)):
            tag = "n=%d k=%d npass=%d q%d %s" % (n, k, c["npass"], qi, sm.spec_name(spec))
            want_idx, want_bits = sm.topk(s, n, k, c["row_base"])
            _check_query(tag, r["idx"][qi], r["bits"][qi], want_idx, want_bits)
            cnt, ti = sm.collect_counts(s, n, kk)
            assert kk <= cnt <= sm.CAP and r["status"][qi] == 0, tag      # (k > n included: kk = n, padding and no status bit)
            assert r["cnt"][qi] == cnt, (tag, r["cnt"][qi], cnt)
            assert tuple(int(x) for x in r["tie_info"][qi]) == ti, (tag, r["tie_info"][qi], ti)


def test_k_beyond_n_pads_and_reports_what_the_model_says(hx):
    """k > n for n <= 8192: the product passes kk = min(k, n), so every row comes back, the slots behind are -1 / -inf and the
    list is not short of kk (status 0); a finalize told kk = k instead reports UNDERFLOW, as the model does."""
    for n, k in ((1, 2), (63, 100), (257, 1000), (1023, 2047), (2047, 2048)):
        specs = sm._family_specs(n, k)[::7][:4]
        arrays = [sm.make_scores(spec, n, 5 + qi) for qi, spec in enumerate(specs)]
        r = hx.exact_select(arrays, n, k)
        for qi, s in enumerate(arrays):
            want_idx, want_bits = sm.topk(s, n, k)
            _check_query("k>n n=%d k=%d q%d" % (n, k, qi), r["idx"][qi], r["bits"][qi], want_idx, want_bits)
            assert (r["idx"][qi][n:] == -1).all() and (r["bits"][qi][n:] == sm.NEG_INF_BITS).all()
            assert r["status"][qi] == 0
        lists = [sm.pack(s, np.arange(n)) for s in arrays]
        idx, bits, st = hx.finalize_lists(lists, [n] * len(lists), k, k)
        for qi, lst in enumerate(lists):
            wi, wb, ws = sm.finalize(lst, n, sm.CAP, k, k)
            _check_query("kk>nc n=%d q%d" % (n, qi), idx[qi], bits[qi], wi, wb)
            assert st[qi] == ws == sm.Q_UNDERFLOW


def test_collect_at_the_capacity_edge(hx):
    """count_gt + ties == 8192: every tie is collected (tie_info[2] == 1, cnt == 8192); one more: the ordered scan keeps the first
    `need` tied rows in row order in the slots [count_gt, count_gt + need)."""
    cases = sm.capacity_cases()
    for i in range(0, len(cases), 3):
        group = cases[i:i + 3]
        n, k = group[0]["n"], group[0]["k"]
        arrays = [sm.make_scores(c["spec"], n, 3) for c in group]
        r = hx.exact_select(arrays, n, k)
        for qi, (c, s) in enumerate(zip(group, arrays)):
            tag = "ties=%d %s" % (c["ties"], sm.spec_name(c["spec"]))
            cnt, ti = sm.collect_counts(s, n, k)
            assert ti[3] == 100 and ti[2] == (1 if c["ties"] == sm.CAP - 100 else 0), tag
            assert r["cnt"][qi] == cnt and tuple(int(x) for x in r["tie_info"][qi]) == ti, (tag, r["cnt"][qi], r["tie_info"][qi], cnt, ti)
            keys = sm.f2key(s)
            above = np.flatnonzero(keys > ti[0])
            tied = np.flatnonzero(keys == ti[0])
            cand = r["cand"][qi]
            if ti[2]:
                assert r["cnt"][qi] == sm.CAP
                assert sorted(cand[:sm.CAP].tolist()) == sorted(sm.pack(s[np.r_[above, tied]], np.r_[above, tied]).tolist()), tag
            else:
                assert r["cnt"][qi] == k
                assert sorted(cand[:100].tolist()) == sorted(sm.pack(s[above], above).tolist()), tag
                assert cand[100:k].tolist() == sm.pack(s[tied[:k - 100]], tied[:k - 100]).tolist(), tag       # in row order
            want_idx, want_bits = sm.topk(s, n, k)
            _check_query(tag, r["idx"][qi], r["bits"][qi], want_idx, want_bits)
            assert r["status"][qi] == 0


# ---- finalize alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threads", sm.THREADS)
def test_finalize_alone_equals_the_model(hx, threads):
    launches = {}
    for c in sm.finalize_cases():
        if c["threads"] == threads:
            launches.setdefault((c["k"], c["kk"], c["inf_status"]), []).append(c)
    seen = set()
    for li, ((k, kk, inf_status), cs) in enumerate(sorted(launches.items())):
        row_base = 2 ** 33 + 5 if li % 5 == 0 else 0
        for c0 in range(0, len(cs), 8):
            part = cs[c0:c0 + 8]
            lists = [sm.make_list(c["layout"], c["nc"], c["kk"], c["seed"]) for c in part]
            qnan = [c["qnan"] for c in part]
            idx, bits, st = hx.finalize_lists(lists, [c["total"] for c in part], k, kk, row_base,
                                              qnan if any(qnan) or li % 2 else None, threads, inf_status)
            for qi, (c, lst) in enumerate(zip(part, lists)):
                tag = "threads=%d %s nc=%d total=%d kk=%d k=%d qnan=%d" % (threads, c["layout"], c["nc"], c["total"], kk, k, c["qnan"])
                wi, wb, ws = sm.finalize(lst, c["total"], sm.CAP, k, kk, row_base, c["qnan"], inf_status)
                _check_query(tag, idx[qi], bits[qi], wi, wb)
                assert st[qi] == ws, (tag, st[qi], ws)
                seen |= sm.branch_labels((lst >> np.uint64(32)).astype(np.uint32), c["total"], sm.CAP, kk, threads)
    assert seen == set(sm.LABELS), sorted(set(sm.LABELS) - seen)


# ---- thresholds -------------------------------------------------------------------------------------------------------------
def _as_float(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("m", sm.SAMPLE_M)
def test_sample_threshold_equals_the_model(hx, m):
    for n in sm.SAMPLE_N:
        arrays = [sm.make_scores(spec, n, 40 + i) for i, spec in enumerate(sm.THRESHOLD_SPECS)]
        thr, cnt, ctr = hx.sample_threshold(arrays, n, m, with_tile_ctr=(n % 2 == 1))
        assert (cnt == 0).all() and ctr in (None, 0), (n, m, cnt, ctr)
        for qi, (spec, s) in enumerate(zip(sm.THRESHOLD_SPECS, arrays)):
            tag = "n=%d m=%d %s" % (n, m, sm.spec_name(spec))
            assert thr[qi] == sm.sample_threshold(s, n, m), (tag, hex(thr[qi]), hex(sm.sample_threshold(s, n, m)))
            if n >= m:                      # the safety property of the filter pass, on its own
                assert _as_float(thr[qi]) <= sm.mth_largest_bits(s, n, m), tag
            else:
                assert thr[qi] == sm.NEG_INF_BITS, tag


@pytest.mark.parametrize("m", sm.RADIX_M)
def test_radix_threshold_equals_the_model(hx, m):
    for n in sm.RADIX_N:
        arrays = [sm.make_scores(spec, n, 60 + i) for i, spec in enumerate(sm.THRESHOLD_SPECS)]
        thr, cnt = hx.radix_threshold(arrays, n, m)
        assert (cnt == 0).all(), (n, m, cnt)
        for qi, (spec, s) in enumerate(zip(sm.THRESHOLD_SPECS, arrays)):
            tag = "n=%d m=%d %s" % (n, m, sm.spec_name(spec))
            assert thr[qi] == sm.radix_threshold(s, n, m), (tag, hex(thr[qi]), hex(sm.radix_threshold(s, n, m)))
            if n >= m:
                assert _as_float(thr[qi]) <= sm.mth_largest_bits(s, n, m), tag
            else:
                assert thr[qi] == sm.NEG_INF_BITS, tag
