"""A numpy model of the selection contract: what hdb_select.hip and hdb_finalize.h must return for a given score array or
candidate list, written as a plain sort.  No GPU and no library: the kernels are compared with this file
(tests/test_select_kernels.py, tests/test_select_end_to_end.py), and this file with a brute-force Python sort
(tests/test_select_model.py).

Contents: the orderable keys of hdb_common.h, the expected outputs of an exact selection (`topk`), of a finalize launch
(`finalize`), of the two threshold kernels (`sample_threshold`, `radix_threshold`), the counters the collect step leaves
(`collect_counts`), the branches of hdb_finalize_fast / hdb_finalize_body a list is designed to take (`branch_labels`, coverage
accounting only), the adversarial score families and the case tables of the kernel tests.
"""
import numpy as np

CAP = 8192                                  # HDB_CAND_CAP: the only capacity the product uses
CNT_STRIDE = 32                             # HDB_CNT_STRIDE
Q_UNDERFLOW, Q_OVERFLOW, Q_NAN = 1, 2, 4
NEG_INF_BITS = np.uint32(0xFF800000)
THREADS = (256, 512, 1024)


# ---- keys ---------------------------------------------------------------------------------------------------------------
def fbits(x):
    """float32 array -> its bits as uint32."""
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32)


def f2key(x):
    """hdb_f2key: ascending uint32 order == float order."""
    u = fbits(x)
    return u ^ np.where((u >> np.uint32(31)) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def key2f(k):
    """hdb_key2f: the float32 of a key."""
    k = np.ascontiguousarray(np.asarray(k, dtype=np.uint32))
    u = k ^ np.where((k >> np.uint32(31)) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    return u.view(np.float32)


def pack(score, row):
    """hdb_pack: (key << 32) | (0xFFFFFFFF - row) as uint64."""
    key = f2key(score).astype(np.uint64)
    r = (np.uint64(0xFFFFFFFF) - np.asarray(row, dtype=np.uint64)).astype(np.uint64)
    return (key << np.uint64(32)) | r


def canon(x):
    """hdb_canon: NaN -> -inf, -0.0 -> +0.0."""
    x = np.array(x, dtype=np.float32, copy=True)
    x[np.isnan(x)] = -np.inf
    return (x + np.float32(0.0)).astype(np.float32)


# ---- expected outputs ---------------------------------------------------------------------------------------------------
def _emit(keys, rows, nout, k, row_base):
    idx = np.full(k, -1, dtype=np.int64)
    bits = np.full(k, NEG_INF_BITS, dtype=np.uint32)
    idx[:nout] = rows[:nout].astype(np.int64) + np.int64(row_base)
    bits[:nout] = fbits(key2f(keys[:nout]))
    return idx, bits


def topk(scores, n, k, row_base=0):
    """One query of an exact selection: rows by (key descending, row ascending), the first min(k, n) of them as
    (int64 row + row_base, float32 score bits); slots beyond are -1 / -inf."""
    keys = f2key(np.asarray(scores, dtype=np.float32)[:n])
    rows = np.arange(n, dtype=np.int64)
    order = np.lexsort((rows, -keys.astype(np.int64)))
    kk = min(k, n)
    return _emit(keys[order], rows[order], kk, k, row_base)


def finalize(entries, total, cap, k, kk, row_base=0, qnan=0, inf_status=0):
    """One query of a finalize launch over a packed candidate list -> (idx, score bits, status)."""
    nc = min(int(total), int(cap))
    e = np.asarray(entries, dtype=np.uint64)[:nc]
    keys = (e >> np.uint64(32)).astype(np.uint32)
    rows = (np.uint64(0xFFFFFFFF) - (e & np.uint64(0xFFFFFFFF))).astype(np.int64)
    order = np.lexsort((rows, -keys.astype(np.int64)))
    idx, bits = _emit(keys[order], rows[order], min(nc, kk), k, row_base)
    st = 0
    if qnan & 2:
        st |= inf_status
    if total > cap:
        st |= Q_OVERFLOW
    if nc < kk:
        st |= Q_UNDERFLOW
    if qnan & 1:
        st |= Q_NAN
    return idx, bits, st


def sample_threshold(scores, n, m):
    """hdb_sample_thr_kernel, exactly: thread t of 1024 keeps the maximum of float4 groups t, t + 1024, ... of the first n/4*4
    scores and of the tail elements n/4*4 + t + 1024 j; the m-th largest of the 1024 maxima (duplicates kept), -inf when n < m or
    when that maximum belongs to a thread that saw nothing.  Returns the float32 bits."""
    keys = f2key(np.asarray(scores, dtype=np.float32)[:n])
    best = np.zeros(1024, dtype=np.uint32)
    n4 = n // 4
    if n4:
        g = keys[:n4 * 4].reshape(n4, 4).max(axis=1)
        pad = np.zeros((n4 + 1023) // 1024 * 1024, dtype=np.uint32)
        pad[:n4] = g
        best = pad.reshape(-1, 1024).max(axis=0)
    for i in range(n4 * 4, n):
        t = (i - n4 * 4) % 1024
        best[t] = max(best[t], keys[i])
    kth = np.sort(best)[::-1][m - 1]
    if n < m or kth == 0:
        return NEG_INF_BITS
    return fbits(key2f(np.array([kth], dtype=np.uint32)))[0]


def radix_threshold(scores, n, m):
    """hdb_thr_kernel after four histogram passes: the m-th largest score, -inf when n < m.  Returns the float32 bits."""
    if n < m:
        return NEG_INF_BITS
    keys = np.sort(f2key(np.asarray(scores, dtype=np.float32)[:n]))[::-1]
    return fbits(key2f(keys[m - 1:m]))[0]


def mth_largest_bits(scores, n, m):
    """The m-th largest score by a plain float sort (no keys): what a threshold may not exceed."""
    s = np.sort(np.asarray(scores, dtype=np.float32)[:n])[::-1]
    return s[m - 1]


def collect_counts(scores, n, kk, cap=CAP):
    """What hdb_launch_collect leaves for one query: (cnt, tie_info[4]) = (candidates appended,
    {k-th key, ties still wanted, ties_all, count_gt})."""
    keys = f2key(np.asarray(scores, dtype=np.float32)[:n])
    kth = np.sort(keys)[::-1][kk - 1]
    count_gt = int((keys > kth).sum())
    ties = int((keys == kth).sum())
    all_ = 1 if count_gt + ties <= cap else 0
    cnt = count_gt + ties if all_ else kk
    return cnt, (int(kth), kk - count_gt, all_, count_gt)


# ---- branch accounting ---------------------------------------------------------------------------------------------------
LABELS = ("fast", "not_fast", "passes_1", "passes_2", "passes_3", "passes_4", "single_keys", "fallback_ns_gt_1024",
          "fallback_ns_gt_threads", "body_preselect", "body_no_preselect", "rank_sort", "bitonic_sort")


def _bin_of_need(h, need):
    """Bins scanned from the top: (bin holding the need-th entry, entries above it, entries in it); (0, 0, 0) when there are fewer."""
    cum = np.cumsum(h[::-1])
    j = int(np.searchsorted(cum, need, side="left"))
    if need == 0 or j >= len(h):
        return 0, 0, 0
    b = len(h) - 1 - j
    return b, int(cum[j] - h[b]), int(h[b])


def branch_labels(keys, total, cap, kk, threads):
    """The branches of hdb_finalize_fast / hdb_finalize_body the list takes: a walk through their control flow (window passes of
    1024 shift bins, the 48-entry rule, the survivor list, the body's 2048-bin pre-selection and its two sorts).  Coverage
    accounting only: no expected value comes from here."""
    nc = min(int(total), int(cap))
    k64 = np.asarray(keys, dtype=np.uint32)[:nc].astype(np.int64)
    out = set()
    fast = 256 < nc <= 16 * threads and 0 < kk <= 256
    if fast:
        out.add("fast")
        lo, hi, need = int(k64.min()), int(k64.max()), kk
        passes, sh, cutoff = 0, 0, lo
        for p in range(4):
            bits = (hi - lo).bit_length()
            sh = max(bits - 10, 0)
            w = k64[(k64 >= lo) & (k64 <= hi)]
            h = np.bincount((w - lo) >> sh, minlength=1024)
            bsel, above, inbin = _bin_of_need(h, need)
            cutoff = lo + (bsel << sh)
            passes = p + 1
            if sh == 0 or inbin <= 48 or p == 3:
                break
            need -= above
            lo, hi = cutoff, min(cutoff + (1 << sh) - 1, hi)
        out.add("passes_%d" % passes)
        if sh == 0:
            out.add("single_keys")
        ns = int((k64 >= cutoff).sum())
        if ns > 1024:
            out.add("fallback_ns_gt_1024")
        if ns > threads:
            out.add("fallback_ns_gt_threads")
        if ns <= 1024 and ns <= threads:
            return out
    else:
        out.add("not_fast")
    ns = nc
    if nc > 512 and kk < nc // 2:
        out.add("body_preselect")
        kmin, kmax = int(k64.min()), int(k64.max())
        sh = max((kmax - kmin).bit_length() - 11, 0)
        b = (k64 - kmin) >> sh
        bsel, _, _ = _bin_of_need(np.bincount(b, minlength=2048), kk)
        ns = int((b >= bsel).sum())
    else:
        out.add("body_no_preselect")
    out.add("rank_sort" if ns <= 256 else "bitonic_sort")
    return out


# ---- score families: (n, seed, ...) -> float32, canonical (no NaN, no -0.0) -----------------------------------------------
def _from_bits(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint32)).view(np.float32).copy()


def one_level(n, seed, value=1.0):
    return np.full(n, value, dtype=np.float32)


def levels(n, seed, sizes=(10,), tie=1, place="spread"):
    """len(sizes) + 1 levels, values len(sizes) + 1 .. 1 from the top; level i holds sizes[i] rows, the last one the rest.  The
    rows of level `tie` (the one meant to hold the k-th) sit: "spread" evenly over the whole array, "last" in the final rows (the
    ordered tie scan walks every chunk before them), "inter" alternating with the other rows from row 0 on."""
    rng = np.random.default_rng(seed)
    cnt, left = [], n
    for s in sizes:                           # (tiny n: a level takes what is left)
        cnt.append(min(int(s), left))
        left -= cnt[-1]
    cnt.append(left)
    vals = [float(len(cnt) - i) for i in range(len(cnt))]
    nt = cnt[tie]
    others = np.concatenate([np.full(c, v, dtype=np.float32) for i, (c, v) in enumerate(zip(cnt, vals)) if i != tie] or
                            [np.zeros(0, dtype=np.float32)])
    rng.shuffle(others)
    pos = np.zeros(n, dtype=bool)
    if place == "spread":
        pos[(np.arange(nt, dtype=np.int64) * n) // max(nt, 1)] = True
    elif place == "last":
        pos[n - nt:] = True
    else:                                     # "inter"
        m = min(nt, n - nt)
        pos[1:2 * m:2] = True
        pos[2 * m:2 * m + (nt - m)] = True
    out = np.empty(n, dtype=np.float32)
    out[pos] = vals[tie]
    out[~pos] = others
    return out


def straddle(n, seed, npos=None, band=0, width=1e-3):
    """Half in [-1, -0.5], half in [0.5, 1] (npos: how many are positive, so the k-th sits on either side of zero); `band` of the
    positive ones lie in the narrow band [0.5, 0.5 + width]."""
    rng = np.random.default_rng(seed)
    npos = n // 2 if npos is None else min(npos, n)
    band = min(band, npos)
    pos = rng.uniform(0.5, 1.0, npos - band).astype(np.float32)
    bnd = (np.float32(0.5) + rng.uniform(0.0, width, band).astype(np.float32)).astype(np.float32)
    neg = (-rng.uniform(0.5, 1.0, n - npos)).astype(np.float32)
    out = np.concatenate([bnd, pos, neg]).astype(np.float32)
    rng.shuffle(out)
    return out


def ulp_chain(n, seed, centre=1.0, byte=0):
    """Scores whose keys differ only in byte `byte`: centre's bits + (i mod 256) << 8 byte, shuffled (byte 0: an np.nextafter
    chain of 256 consecutive floats away from zero)."""
    rng = np.random.default_rng(seed)
    base = int(fbits(np.float32(centre)).reshape(-1)[0]) & ~(0xFF << (8 * byte))       # (byte 2 of +-1.0 is 0x80: the chain runs 0.5 .. 2)
    b = (base + ((np.arange(n, dtype=np.int64) % 256) << (8 * byte))).astype(np.uint32)
    out = _from_bits(b)
    rng.shuffle(out)
    return out


def denormals(n, seed):
    """Denormals and tiny normals of both signs, mixed with 0.0."""
    rng = np.random.default_rng(seed)
    mag = rng.integers(1, 0x01800000, n, dtype=np.int64)          # denormals (below 0x00800000) and the first normal binades
    mag[rng.random(n) < 0.4] &= 0xFF                               # many in the lowest byte: 1 .. 255 ulps of zero
    sign = rng.integers(0, 2, n, dtype=np.int64) << 31
    out = _from_bits((mag | sign).astype(np.uint32))
    out[rng.random(n) < 0.2] = 0.0
    return canon(out)


def full_range(n, seed):
    """+-3e38 down to 1e-30: every exponent bin populated."""
    rng = np.random.default_rng(seed)
    e = rng.integers(27, 255, n, dtype=np.int64)                    # biased exponents: 2^-100 .. 2^127
    man = rng.integers(0, 1 << 23, n, dtype=np.int64)
    sign = rng.integers(0, 2, n, dtype=np.int64) << 31
    out = _from_bits((sign | (e << 23) | man).astype(np.uint32))
    return np.clip(out, -3e38, 3e38).astype(np.float32)


def inf_mix(n, seed, nfinite=None, nposinf=1):
    """+-inf as real scores: nposinf rows at +inf, nfinite finite ones, the rest at -inf (a k beyond nposinf + nfinite reaches
    into the -inf rows)."""
    rng = np.random.default_rng(seed)
    nposinf = min(nposinf, n)
    nfinite = (n - nposinf) // 2 if nfinite is None else min(nfinite, n - nposinf)
    out = np.full(n, -np.inf, dtype=np.float32)
    out[:nposinf] = np.inf
    out[nposinf:nposinf + nfinite] = rng.standard_normal(nfinite).astype(np.float32)
    rng.shuffle(out)
    return canon(out)


def int_levels(n, seed, d=8):
    """Integer levels 0 .. d, as hamming produces them (binomial around d / 2)."""
    rng = np.random.default_rng(seed)
    return rng.binomial(d, 0.5, n).astype(np.float32)


def gaussian(n, seed):
    return canon(np.random.default_rng(seed).standard_normal(n).astype(np.float32))


FAMILIES = {"one_level": one_level, "levels": levels, "straddle": straddle, "ulp_chain": ulp_chain, "denormals": denormals,
            "full_range": full_range, "inf_mix": inf_mix, "int_levels": int_levels, "gaussian": gaussian}


def hamming_npass(d):
    """The radix passes plan_topk chooses for hamming scores of a d-bit index (hdb_plan.h): min(4, (8 + bits(d) + 7) / 8)."""
    bits = 0
    while (d >> bits) != 0:
        bits += 1
    return min(4, (8 + bits + 7) // 8)


def arrange(scores, order, seed):
    """The same multiset of scores placed by row: "asc", "desc", "shuf", or None (as the family built it)."""
    s = np.asarray(scores, dtype=np.float32)
    if order == "asc":
        return np.sort(s)
    if order == "desc":
        return np.sort(s)[::-1].copy()
    if order == "shuf":
        return np.random.default_rng(seed + 977).permutation(s)
    return s.copy()


def make_scores(spec, n, seed):
    """spec = (family name, parameter dict, order) -> the float32 score array of n rows."""
    name, params, order = spec
    s = FAMILIES[name](n, seed, **params)
    assert s.dtype == np.float32 and s.shape == (n,)
    return arrange(s, order, seed)


def spec_name(spec):
    name, params, order = spec
    p = ",".join("%s=%s" % (a, params[a]) for a in sorted(params))
    return "%s(%s)%s" % (name, p, ":" + order if order else "")


# ---- case table 1: exact selection (hist x npass, collect, finalize) -------------------------------------------------------
EXACT_N = (1, 63, 255, 256, 257, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 8256, 20011)
EXACT_K = (1, 2, 16, 17, 100, 256, 257, 1000, 2047, 2048)


def _family_specs(n, k):
    """Every family at (n, k), the k-dependent parameters chosen so that the k-th lands where the family wants it."""
    kk = min(k, n)
    top = max(kk // 2, 0)                      # rows above the level of the k-th
    specs = []
    for v in (0.0, 1.0, float("inf"), float("-inf")):
        specs.append(("one_level", {"value": v}, None))
    for place in ("spread", "last", "inter"):
        specs.append(("levels", {"sizes": (top,), "tie": 1, "place": place}, None))                       # two levels
        specs.append(("levels", {"sizes": (top, max(n // 2, kk - top)), "tie": 1, "place": place}, None))    # three, the k-th in the middle
    for order in ("asc", "desc", "shuf"):
        specs.append(("straddle", {"npos": n // 2, "band": 0}, order))                  # the k-th on the positive side (k <= n / 2)
        specs.append(("straddle", {"npos": max(kk // 3, 0), "band": 0}, order))        # ... on the negative side
        specs.append(("straddle", {"npos": kk // 2 + 600, "band": 600}, order))        # the k-th among 600 in one narrow band
        for centre in (1.0, -1.0):
            for byte in (0, 1, 2):
                specs.append(("ulp_chain", {"centre": centre, "byte": byte}, order))
        specs.append(("denormals", {}, order))
        specs.append(("full_range", {}, order))
        specs.append(("inf_mix", {"nfinite": max(kk // 2, 0), "nposinf": min(3, kk)}, order))   # k reaches into the -inf rows
        specs.append(("inf_mix", {}, order))
        specs.append(("gaussian", {}, order))
        for d in (8, 40, 384):
            specs.append(("int_levels", {"d": d}, order))
    return specs


# (n, k) pairs: every n and every k of the issue's lists, each boundary n with the k around it
EXACT_PAIRS = (
    (1, 1), (1, 2), (63, 16), (63, 100), (255, 17), (255, 256), (256, 256), (256, 257), (257, 256), (257, 257), (257, 1000),
    (1023, 1), (1023, 1000), (1024, 2), (1024, 2047), (1025, 100), (1025, 1000), (4097, 16), (4097, 2047), (4097, 2048),
    (8191, 17), (8191, 2048), (8192, 1), (8192, 256), (8192, 2048), (8193, 2), (8193, 257), (8193, 2047), (8256, 100),
    (8256, 1000), (8256, 2048), (20011, 1), (20011, 16), (20011, 17), (20011, 100), (20011, 256), (20011, 257), (20011, 1000),
    (20011, 2047), (20011, 2048),
)
QUERIES_PER_LAUNCH = 4


def exact_cases():
    """The launches of the exact-selection test: dicts {n, k, npass, row_base, specs (3-4 families), seed}.  The families rotate
    through the (n, k) pairs so that every family meets small, boundary and large sizes; hamming levels ride launches of their
    own with the plan's npass (the other families need all four passes)."""
    cases, rot = [], 0
    nspec = len(_family_specs(8, 1))
    for i, (n, k) in enumerate(EXACT_PAIRS):
        specs = _family_specs(n, k)
        general = [s for s in specs if s[0] != "int_levels"]
        take = QUERIES_PER_LAUNCH * (3 if n >= 8192 else 2)       # two or three launches per pair
        for j in range(0, take, QUERIES_PER_LAUNCH):
            pick = [general[(rot + j + t) % len(general)] for t in range(QUERIES_PER_LAUNCH)]
            cases.append({"n": n, "k": k, "npass": 4, "row_base": 0, "specs": pick, "seed": 1000 * i + j})
        rot += take + 1
    assert nspec == len(_family_specs(20011, 2048))
    # hamming levels: the plan's npass and 4, at sizes around the tile and capacity boundaries
    for i, (n, k) in enumerate(((257, 16), (1025, 100), (8193, 257), (20011, 1000), (20011, 2048))):
        for d in (8, 40, 384):
            pick = [("int_levels", {"d": d}, o) for o in ("asc", "desc", "shuf")] + [("one_level", {"value": 1.0}, None)]
            for npass in sorted({hamming_npass(d), 4}):
                cases.append({"n": n, "k": k, "npass": npass, "row_base": 0, "specs": pick, "seed": 50000 + 10 * i + d})
    # a row base beyond 2^33
    cases.append({"n": 8193, "k": 100, "npass": 4, "row_base": 2 ** 33 + 5, "seed": 7,
                  "specs": [("gaussian", {}, "shuf"), ("levels", {"sizes": (50,), "tie": 1, "place": "last"}, None),
                            ("straddle", {"npos": 30, "band": 0}, "shuf"), ("ulp_chain", {"centre": -1.0, "byte": 0}, "shuf")]})
    # ties beyond the candidate capacity: the ordered tie scan, with the tied rows in each placement
    for n, k, top in ((20011, 100, 40), (20011, 2048, 1000), (8256, 257, 0), (20011, 1, 0)):
        pick = [("levels", {"sizes": (top,), "tie": 1, "place": p}, None) for p in ("spread", "last", "inter")]
        pick.append(("levels", {"sizes": (top, n - top - 300), "tie": 1, "place": "last"}, None))
        cases.append({"n": n, "k": k, "npass": 4, "row_base": 0, "specs": pick, "seed": 90000 + n + k})
    return cases


def capacity_cases():
    """Collect at the capacity edge: n = 8256, 100 rows above, then 8092 (fits: 8192 in all) or 8093 (one too many: the ordered
    scan) tied rows holding the k-th, the rest below."""
    out = []
    for ties in (CAP - 100, CAP - 99):
        for place in ("spread", "last", "inter"):
            out.append({"n": 8256, "k": 200, "spec": ("levels", {"sizes": (100, ties), "tie": 1, "place": place}, None), "ties": ties})
    return out


# ---- case table 2: finalize alone -----------------------------------------------------------------------------------------
def _unique_rows(rng, nc):
    return rng.permutation(np.arange(3 * nc + 7, dtype=np.int64))[:nc]


def layout_keys(layout, nc, kk, seed):
    """The score array (float32, nc entries) of a finalize key layout."""
    rng = np.random.default_rng(seed)
    if layout == "uniform":                   # one positive binade: 1024 even bins, one pass
        return rng.uniform(1.0, 2.0, nc).astype(np.float32)
    if layout == "gauss":
        return gaussian(nc, seed)
    if layout == "straddle2":                 # half below zero, the rest spread over [0.5, 1]: the second pass separates them
        return straddle(nc, seed, npos=nc // 2, band=0)
    if layout == "straddle3":                 # ... with all but 8 of the positive ones in a 2e-4 band (3355 keys, inside one 4096-key bin of
        return straddle(nc, seed, npos=nc // 2, band=nc // 2 - 8, width=2e-4)       # the second pass) that holds the kk-th: a third pass
    if layout == "straddle4":                 # ... and the kk-th among 4 adjacent keys that 400+ entries share: a fourth pass (8 entries
        s = straddle(nc, seed, npos=nc // 2, band=nc // 4)          # far above keep every window at its full width); kk >= 16
        order = np.argsort(-s, kind="stable")
        s[order[:8]] = rng.uniform(2.0, 4.0, 8).astype(np.float32)
        end = min(kk + 400, nc // 2 - 1)                            # (stays among the positive ones)
        grp = order[8:end]
        base = int(fbits(np.float32(s[order[end]])).reshape(-1)[0]) & ~3
        s[grp] = _from_bits((base + rng.integers(0, 4, len(grp))).astype(np.uint32))
        return s
    if layout == "ulp":                       # consecutive keys: single-key bins in the first pass
        return ulp_chain(nc, seed, centre=1.0, byte=0)
    if layout == "equal":
        return np.full(nc, 1.5, dtype=np.float32)
    if layout == "ties300":                   # 300 equal keys around the kk-th, the others distinct
        s = rng.uniform(1.0, 2.0, nc).astype(np.float32)
        order = np.argsort(-s, kind="stable")
        lo = max(min(kk, nc) - 150, 0)
        grp = order[lo:lo + 300]
        s[grp] = s[order[min(kk, nc) - 1]]
        return s
    if layout == "inf_mix":
        return inf_mix(nc, seed)
    if layout == "denormals":
        return denormals(nc, seed)
    raise KeyError(layout)


def make_list(layout, nc, kk, seed):
    """A packed candidate list of nc entries in shuffled order, rows unique."""
    rng = np.random.default_rng(seed + 31)
    s = layout_keys(layout, nc, kk, seed) if nc else np.zeros(0, dtype=np.float32)
    return pack(s, _unique_rows(rng, nc))


FIN_NC = (0, 1, 2, 255, 256, 257, 511, 512, 513, 1024, 1025, 4096, 4097, 8191, 8192)


def finalize_cases():
    """The queries of the finalize test: dicts {threads, layout, nc, total, kk, k, qnan, inf_status, seed}.  Grouped into launches
    by (threads, k, kk, inf_status) in the test.  The same table at 256, 512 and 1024 threads."""
    rows = []

    def add(layout, nc, kk, total=None, qnan=0, inf_status=0):
        rows.append({"layout": layout, "nc": nc, "total": nc if total is None else total, "kk": kk, "qnan": qnan,
                     "inf_status": inf_status})

    # every nc with every fixed kk it can serve, on the one-pass layout and on gaussian keys (which straddle zero)
    for nc in FIN_NC:
        kks = {1, 16, 255, 256, 257, 2048}
        if nc // 2 - 1 >= 1:
            kks |= {nc // 2 - 1, nc // 2}
        for kk in sorted(kks):
            add("uniform" if (nc + kk) % 2 else "gauss", nc, kk)        # (kk > nc among them: underflow)
    # overflow: the counter says 8192 + 5, the list holds 8192
    for kk in (1, 16, 256, 257, 2048):
        add("uniform", CAP, kk, total=CAP + 5)
        add("straddle2", CAP, kk, total=CAP + 5)
    # the window passes, the survivor fallbacks and the body's branches
    for nc in (513, 1025, 4096, 4097, 8192):
        for kk in (16, 100, 256):
            add("straddle2", nc, kk)
            add("straddle3", nc, kk)
            add("straddle4", nc, kk)
            add("ulp", nc, kk)
            add("ties300", nc, kk)
    add("straddle4", 4096, 150)
    add("equal", 3000, 16)
    add("equal", 3000, 256)
    add("equal", 3000, 1000)
    add("ties300", 2000, 257)
    add("ties300", 4097, 1000)
    add("inf_mix", 1025, 256)
    add("inf_mix", 4097, 2048)
    add("denormals", 1025, 16)
    add("denormals", 8191, 257)
    add("ulp", 255, 16)
    add("ulp", 8192, 2048)
    # status flags: qnan 0..3 with both inf_status values
    for inf_status in (0, Q_UNDERFLOW):
        for qnan in (0, 1, 2, 3):
            add("uniform", 1025, 16, qnan=qnan, inf_status=inf_status)
            add("gauss", 100, 16, qnan=qnan, inf_status=inf_status)
    add("uniform", 8, 16, qnan=3, inf_status=Q_UNDERFLOW)            # underflow from the list and from the flag at once
    out = []
    for threads in THREADS:
        for i, r in enumerate(rows):
            c = dict(r)
            c["threads"] = threads
            c["k"] = c["kk"] + 2                    # (two padding slots behind the kk results)
            c["seed"] = 100 + i
            out.append(c)
    return out


# what a layout is built for wherever the fast path takes the list (256 < nc <= 16 * threads, 16 <= kk <= 256)
LAYOUT_BUILT_FOR = {"uniform": {"passes_1"}, "straddle2": {"passes_2"}, "straddle3": {"passes_3"}, "straddle4": {"passes_4", "single_keys"},
                    "ulp": {"passes_1", "single_keys"}, "equal": {"fallback_ns_gt_1024", "body_preselect", "bitonic_sort"}}


def finalize_case_labels(c):
    lst = make_list(c["layout"], c["nc"], c["kk"], c["seed"])
    keys = (lst >> np.uint64(32)).astype(np.uint32)
    return branch_labels(keys, c["total"], CAP, c["kk"], c["threads"])


# ---- case table 3: thresholds ---------------------------------------------------------------------------------------------
SAMPLE_M = (1, 2, 15, 16)
SAMPLE_N = (1, 3, 4, 5, 1023, 1024, 1025, 4099, 20011)
RADIX_M = (17, 100, 1000)
RADIX_N = (16, 99, 257, 1025, 4099, 20011)
THRESHOLD_SPECS = (
    ("gaussian", {}, "shuf"), ("straddle", {"band": 0}, "asc"), ("straddle", {"band": 300}, "shuf"),
    ("ulp_chain", {"centre": 1.0, "byte": 0}, "shuf"), ("ulp_chain", {"centre": -1.0, "byte": 1}, "desc"),
    ("inf_mix", {}, "shuf"), ("inf_mix", {"nfinite": 5, "nposinf": 2}, "asc"), ("one_level", {"value": float("-inf")}, None),
    ("denormals", {}, "shuf"), ("full_range", {}, "desc"), ("levels", {"sizes": (3,), "tie": 1, "place": "last"}, None),
)


# ---- the coverage table (profiles/select_coverage.txt) ----------------------------------------------------------------------
def coverage_text():
    lines = ["# Selection kernel tests: the case tables of tests/select_model.py and the branches each case is built for.",
             "# Generated by `python tests/select_model.py`; tests/test_select_model.py fails when this file is out of date.",
             "", "## finalize alone (hdb_launch_finalize): layout nc total kk threads -> branch labels"]
    seen = {t: set() for t in THREADS}
    for c in finalize_cases():
        lab = finalize_case_labels(c)
        seen[c["threads"]] |= lab
        if c["qnan"] or c["inf_status"]:
            continue                              # (the status-flag cases repeat the layouts above them)
        lines.append("%-10s nc=%-5d total=%-5d kk=%-5d threads=%-5d %s" % (c["layout"], c["nc"], c["total"], c["kk"], c["threads"],
                                                                         " ".join(sorted(lab))))
    lines += ["", "## labels covered per thread count"]
    for t in THREADS:
        lines.append("threads=%d: %s" % (t, " ".join(l for l in LABELS if l in seen[t])))
        lines.append("threads=%d missing: %s" % (t, " ".join(l for l in LABELS if l not in seen[t]) or "none"))
    lines += ["", "## exact selection (hist x npass, collect, finalize at 1024 threads): n k npass row_base | families -> labels of each query's"
              " candidate list"]
    for c in exact_cases():
        labs = []
        for qi, spec in enumerate(c["specs"]):
            s = make_scores(spec, c["n"], c["seed"] + qi)
            kk = min(c["k"], c["n"])
            cnt, _ = collect_counts(s, c["n"], kk)
            keys = np.sort(f2key(s))[::-1][:cnt]
            labs.append("%s -> nc=%d %s" % (spec_name(spec), cnt, " ".join(sorted(branch_labels(keys, cnt, CAP, kk, 1024)))))
        lines.append("n=%-5d k=%-4d npass=%d row_base=%d" % (c["n"], c["k"], c["npass"], c["row_base"]))
        lines += ["    " + l for l in labs]
    lines += ["", "## collect at the capacity edge: n k ties placement"]
    for c in capacity_cases():
        lines.append("n=%d k=%d ties=%d %s" % (c["n"], c["k"], c["ties"], spec_name(c["spec"])))
    lines += ["", "## thresholds", "sample threshold: m in %s, n in %s" % (SAMPLE_M, SAMPLE_N),
              "radix threshold: m in %s, n in %s" % (RADIX_M, RADIX_N), "families:"]
    lines += ["    " + spec_name(s) for s in THRESHOLD_SPECS]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "select_coverage.txt")
    with open(path, "w") as f:
        f.write(coverage_text())
    print("wrote", path)
