"""Conditions on the SCHEDULES of tests/test_lifecycle_model.py, checked on the CPU: what the GPU test covers is asserted here on the step
lists themselves (tests/lifecycle_model.py), for every (case, seed) it runs, so coverage is a condition and not luck; and the model's
own expectations are sane -- planted rows score as designed in float64, and no top-k probe sits where check_topk could fail a correct
kernel.  Nothing here looks at the code under test."""
import numpy as np
import pytest

import lifecycle_model as lm

RUNS = [(case, seed) for case in lm.CASES for seed in lm.SEEDS]
MUTATIONS = ("append", "poison_nan", "poison_inf", "compact", "heal", "update")


def _has(probe, metrics):
    return all(m in lm.PROBES[probe] for m in metrics)


@pytest.mark.parametrize("case,seed", RUNS)
def test_schedule_covers_what_it_is_meant_to(case, seed):
    c = lm.CASES[case]
    S = lm.schedule(case, seed)
    assert len(S) <= lm.MAX_STEPS
    assert all(1 <= st["n0"] <= lm.N_MAX and 1 <= st["n1"] <= lm.N_MAX for st in S)
    ops = {st["op"] for st in S}
    want = {"append", "compact", "update", "set_bias", "set_mask", "set_subset"}
    want |= {"quantize_on", "quantize_off"} if c["shadow"] else set()
    want |= {"poison_nan", "heal"} if c["nan"] else set()
    want |= {"poison_inf", "heal"} if c["inf"] else set()
    assert ops == want, ops ^ want
    assert {st["probe"] for st in S} == set(lm.PROBES)
    appends = [st for st in S if st["op"] == "append"]
    kinds = {st["kind"] for st in appends}
    assert kinds == set(lm.APPEND_KINDS) - (set() if c["shadow"] else {"past_shadow"}), kinds
    assert {st["kind"] for st in S if st["op"] == "compact"} == set(lm.COMPACT_KINDS)
    sizes = [st["m"] for st in S if st["op"] == "update"]
    n_before = [st["n0"] for st in S if st["op"] == "update"]
    assert any(m > n for m, n in zip(sizes, n_before)) and any(m < n for m, n in zip(sizes, n_before))
    assert all(st["m"] <= 2000 for st in appends if st["kind"] == "random")
    # appends against the 256-row blocks of the sign bits and the capacities valid at that moment
    assert any(st["m"] == 1 and st["n0"] % 256 not in (0, 255) and st["n1"] % 256 not in (0, 255) for st in appends)
    assert any(st["n1"] % 256 == 0 for st in appends)
    assert any(st["n0"] <= st["cache_rows"] < st["n1"] for st in appends)
    assert any(st["bits_cap"] > 0 and lm._align(max(st["n0"], 4), 256) <= st["bits_cap"] < lm._align(max(st["n1"], 4), 256) for st in appends)
    if c["shadow"]:
        assert any(st["quant"] and st["n0"] <= st["q_rows"] < st["n1"] for st in appends)
    # orders
    for i, st in enumerate(S[:-1]):
        if st["op"] in ("compact", "heal") and st["probe"] == "none" and S[i + 1]["op"] == "append":
            break
    else:
        raise AssertionError("no append right behind a compaction")
    assert any(st["op"] == "append" and st["n0"] <= lm.CAND_CAP < st["n1"] for st in S)
    assert any(st["op"] == "compact" and st["n1"] <= lm.CAND_CAP < st["n0"] for st in S)
    for seen, metrics in (("bits_seen", lm.BITS), ("pearson_seen", lm.PEARSON)):
        ok = False
        for i, st in enumerate(S):
            if st["op"] == "compact" and st[seen] is not None and st["n1"] < st[seen] and not _has(st["probe"], metrics):
                j = next((j for j in range(i + 1, len(S)) if S[j]["op"] == "append"), None)
                gap = [] if j is None else S[i + 1:j]
                if j is not None and not any(_has(x["probe"], metrics) or x["op"] == "update" for x in gap):
                    nxt = next((x for x in S[j:] if x["op"] == "update" or _has(x["probe"], metrics)), None)
                    ok |= nxt is not None and _has(nxt["probe"], metrics) and nxt["op"] != "update"
        assert ok, seen
    if c["shadow"]:
        off = [i for i, st in enumerate(S) if st["op"] == "quantize_off"]
        assert any(st["op"] == "quantize_on" for st in S[off[0] + 1:])
        assert any(S[i - 1]["op"] in ("compact", "heal") for i in off), "quantize(None) right after a compaction"
        # ... and probes that can take the shadow: dense metrics on more than CAND_CAP finite rows while a shadow exists
        hits = sum(st["probe"] in ("dense", "all") and st["n1"] > lm.CAND_CAP and not st["op"].startswith("poison") and bool(S[i + 1]["quant"])
                   for i, st in enumerate(S[:-1]))                # (a step's "quant" is the state before its op: the next step's tells this one's)
        assert hits >= 2
    for name in ("set_bias", "set_mask", "set_subset"):
        i = next(i for i, st in enumerate(S) if st["op"] == name)
        assert st_probes_dense(S[i]), name                      # the input is used before it is dropped ...
        j = next(j for j in range(i + 1, len(S)) if S[j]["op"] in MUTATIONS)
        assert not any(S[x]["op"].startswith("set_") for x in range(i + 1, j))
        assert any(S[x]["probe"] != "none" for x in range(j, len(S))) and S[j]["probe"] in ("dense", "all"), name
    seq = [st["op"] for st in S if st["op"] in ("poison_nan", "poison_inf", "heal")]
    assert seq == (["poison_nan", "heal"] if c["nan"] else []) + (["poison_inf", "heal"] if c["inf"] else [])
    for i, st in enumerate(S):
        if st["op"].startswith("poison"):
            assert st["probe"] == "all" and S[i + 1]["op"] == "heal" and S[i + 1]["probe"] == "all"
    # update to a smaller matrix with every lazy cache warm
    assert any(st["op"] == "update" and st["m"] < st["n0"] and S[i - 1]["probe"] == "all" for i, st in enumerate(S) if i)
    assert S[-1]["probe"] == "all"


def st_probes_dense(st):
    return st["probe"] in ("dense", "all")


def test_schedules_are_deterministic_and_differ_by_seed():
    a, b = lm.schedule("f32", 1), lm.schedule("f32", 1)
    assert [(x["op"], x["probe"], x["n1"]) for x in a] == [(x["op"], x["probe"], x["n1"]) for x in b]
    assert [x["n1"] for x in a] != [x["n1"] for x in lm.schedule("f32", 2)]
    long = lm.random_schedule("f16-plane", 3, 120)
    assert len(long) == 120 and all(1 <= x["n1"] <= lm.N_MAX for x in long) and long[-1]["probe"] == "all"


def test_pinned_reductions_are_short_and_in_range():
    for name in lm.PINNED:
        case, seed, steps = lm.pinned_schedule(name)
        assert case in lm.CASES and len(steps) <= 4 and all(1 <= st["n1"] <= lm.N_MAX for st in steps) and steps[-1]["probe"] != "none"
    _, _, steps = lm.pinned_schedule("masked_rows_in_the_full_sort")
    assert steps[-1]["op"] == "set_mask" and steps[-1]["n1"] > max(lm.CAND_CAP, 2048)          # k = n takes the full sort, under a mask


def test_capacity_rules_of_the_model():
    """Caps restates hdb_api.hip: the numbers of its comments, on the sizes the existing tests name."""
    c = lm.Caps(9000, "explicit")
    assert c.cache_rows == 9000 + 2250 + 64 and c.q_rows == 9000 + 4500 + 64          # test_extend_to_the_last_row_of_the_capacity
    assert not c.append(c.q_rows - 9000)["shadow"] and c.append(1)["shadow"]
    c = lm.Caps(300, None)
    c.probe("bits")
    assert c.bits_cap == 768 and c.bits_seen == 300
    assert not c.append(468)["bits"] and c.append(1)["bits"]
    c.compact(10)
    assert c.cache_rows == 10 + 2 + 64 and c.bits_cap == 768
    a = lm.Caps(9000, "auto")
    a.probe("bits")
    assert a.quant is None
    a.probe("dense")
    assert a.quant == "auto" and a.q_rows == 9064 and a.append(65)["shadow"]


@pytest.mark.parametrize("case,seed", RUNS)
def test_model_expectations_are_sane(case, seed):
    """The planted rows score as designed in float64 (NaN exactly where planted), and no top-k probe has its k-th and (k+1)-th exact
    scores further apart than check_topk's slack yet within the rounding noise of a correct float32 kernel."""
    from oracle import ranking_oracle as orc
    c = lm.CASES[case]
    m = lm.Model(case, seed)
    Q = m.data.Q
    hazards, probes = [], 0

    def planted_ok():
        lo, pl = m.planted_at
        if not pl:
            return
        V64 = m.V.astype(np.float64)
        assert np.array_equal(V64[lo + pl["query0"]], Q[0].astype(np.float64))
        assert np.array_equal(V64[lo + pl["dup"][0]], V64[lo + pl["dup"][1]])
        assert not V64[lo + pl["zero"]].any() and np.ptp(V64[lo + pl["const"]]) == 0 and V64[lo + pl["const"], 0] != 0
        blk = slice(lo, m.n)
        for metric in lm.PROBES["all"]:
            ref, nan = lm.expected_scores(orc, V64[blk], Q[0], metric)
            want = np.zeros(m.n - lo, dtype=bool)
            if metric == "pearson_correlation":
                want[[pl["zero"], pl["const"]]] = True
                if c["storage"] in ("float8", "int8"):           # a row scaled down may round to a constant (zero) row in these formats
                    want |= np.ptp(V64[blk], axis=1) == 0
            if m.poison is not None and metric not in ("hamming_distance", "jaccard_similarity") and m.poison[1] >= lo:
                if m.poison[0] == "nan" or metric in ("cosine_similarity", "pearson_correlation"):
                    want[m.poison[1] - lo] = True
            assert np.array_equal(nan, want), (metric, np.flatnonzero(nan != want)[:5])
            rest = ref[~nan]
            if m.poison is None:
                assert np.isfinite(rest).all(), metric
        s = lm.expected_scores(orc, V64[blk], Q[0], "cosine_similarity")[0]
        assert abs(s[pl["query0"]] - 1.0) < 1e-12 and s[pl["zero"]] == 0.0

    planted_ok()
    for st in lm.schedule(case, seed):
        m.apply(st)
        if st["op"] in ("append", "update"):
            planted_ok()
        metrics = lm.PROBES[st["probe"]]
        if not metrics or np.isnan(m.V).any():
            continue
        V64 = m.V.astype(np.float64)
        part = np.arange(m.n) if m.mask is None else np.flatnonzero(m.mask)
        if m.poison is not None:
            part = part[part != m.poison[1]]
        for metric in metrics:
            tol = lm.tol_of(c["storage"], metric)
            if m.bias is not None and tol == 0.0:
                tol = 1e-5
            for qi in range(lm.NQ):
                ref = lm.expected_scores(orc, V64, Q[qi], metric)[0]
                if m.bias is not None:
                    ref = ref + m.bias
                ref = ref[part]
                for k in sorted({1, min(100, m.n)}):
                    if k >= ref.size:
                        continue
                    probes += 1
                    kth = np.sort(ref[np.isfinite(ref)])[::-1][k - 1] if np.isfinite(ref).sum() >= k else 0.0
                    if lm.tie_hazards(ref, k, tol, lm.f32_noise(metric, c["d"], kth, c["storage"])):
                        hazards.append((st["op"], st["probe"], metric, qi, k))
    print(f"{case} seed {seed}: {probes} top-k boundaries, {len(hazards)} inside the hazard band")
    assert probes > 100 and not hazards, hazards[:5]
