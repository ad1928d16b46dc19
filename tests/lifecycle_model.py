"""Host model of a long-lived GpuIndex and the schedules that tests/test_lifecycle_model.py drives through it.

Every storage type keeps per-row state beside the matrix (1/|v| and |v|^2 with head room, the NaN / INF flag word, lazily packed sign
bits, lazily computed pearson scales, the int8 shadow with its 5-bit plane, borrowed bias / mask / row list) and every mutation keeps
that state up incrementally.  The model here is the matrix alone -- the STORED values widened exactly, what GpuIndex.host_matrix()
returns -- plus the per-row inputs that are live and a row-count simulation of the library's capacities (Caps), so a schedule can aim
an append at "one row past the head room that holds right now".  Everything a probe expects is computed from the model's matrix by
oracle/ranking_oracle.py in float64, or by a FRESH index registered over that matrix.

schedule(case, seed) is a deterministic list of steps {op, probe}; tests/test_lifecycle_inputs.py asserts on the CPU that each list
covers what it is meant to cover.  run(case, seed) applies a list to the model and to one GpuIndex and checks every probed step.

A plain module like tests/lowscore.py.  Command line (needs the GPU): python tests/lifecycle_model.py STEPS SEED [CASE] runs a random
schedule of STEPS steps and prints the first failing step as a (case, seed, step) triple; replay(case, seed, step) runs up to it.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "local-hyperdb_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

CAND_CAP = 8192                        # HDB_CAND_CAP: up to this many rows a call is "small" (no sampled threshold, no shadow)
N_MAX = 12_000
MAX_STEPS = 36
SEEDS = (1, 2)
NQ = 6
DENSE = ("dot_product", "cosine_similarity", "euclidean_metric", "manhattan_distance")
BITS = ("hamming_distance", "jaccard_similarity")
PEARSON = ("pearson_correlation",)
PROBES = {"none": (), "dense": DENSE, "bits": BITS, "pearson": PEARSON, "all": DENSE + BITS + PEARSON}
APPEND_KINDS = ("1", "3", "15", "16", "17", "255", "256", "257", "to256", "past_head", "past_shadow", "random")
COMPACT_KINDS = ("identity", "but_first", "but_last", "single", "prefix", "suffix", "half", "sixteenth")

# storage, d, the shadow the index carries, whether a NaN / an infinite element can be stored
CASES = {
    "f16-plane": dict(id=0, storage="float16", d=384, shadow="explicit", nan=True, inf=True),
    "f16-auto": dict(id=1, storage="float16", d=384, shadow="auto", nan=True, inf=True),
    "f16-odd": dict(id=2, storage="float16", d=72, shadow=None, nan=True, inf=True),
    "f32": dict(id=3, storage="float32", d=100, shadow="explicit", nan=True, inf=True),
    "bf16": dict(id=4, storage="bfloat16", d=96, shadow="explicit", nan=True, inf=True),
    "f8": dict(id=5, storage="float8", d=128, shadow=None, nan=True, inf=False),
    "i8": dict(id=6, storage="int8", d=40, shadow=None, nan=False, inf=False),
    "f64": dict(id=7, storage="float64", d=33, shadow=None, nan=True, inf=True),
}
F8_MAX = 448.0


def tol_of(storage, metric):
    """The project's score contract (tests/test_gpu_parity.py _tol): tol * max(1, |s|)."""
    if metric == "hamming_distance":
        return 0.0
    if metric == "jaccard_similarity":
        return 1e-6
    return 1e-3 if storage == "float16" else 1e-5


def _align(x, a):
    return (x + a - 1) // a * a


# ---- the library's capacities as functions of the row counts it has seen (hdb_api.hip) ---------------------------------------------
class Caps:
    """Row counts only.  cache_rows (inv_norm.cap): build_caches n + n/4 + 64 (kept when the new matrix fits), hdb_index_extend
    n + n/2 + 64 when it grows, hdb_index_gather m + m/4 + 64.  bits_cap: ensure_bits, align_up(npad + npad/4, 256) over
    npad = align_up(max(n, 4), 256), reallocated by the bit-metric call that finds it short, never shrunk.  q_rows: quant_room
    need + need/2 + 64 (the automatic build need + 64), the gather's m + m/4 + 64; an automatic shadow is built by the first
    1-4-query dot / cosine top-k on more than CAND_CAP finite rows."""

    def __init__(self, n, shadow):
        self.n, self.kind = n, shadow
        self.cache_rows = n + n // 4 + 64
        self.bits_cap, self.bits_seen, self.pearson_seen = 0, None, None
        self.quant, self.q_rows, self.auto_armed = None, 0, shadow == "auto"
        self.poison = None                 # None | ("nan" | "inf", row)
        if shadow == "explicit":
            self.quantize(True)

    def _reserve(self, need, tight=False):
        need = max(need, 1)
        if not (self.q_rows and need <= self.q_rows):
            self.q_rows = need + 64 if tight else need + need // 2 + 64

    def quantize(self, on):
        if on:
            self._reserve(self.n)
            self.quant = "explicit"
        else:
            self.quant, self.q_rows, self.auto_armed = None, 0, False

    def append(self, m):
        """-> which capacities the append crosses (head room, bit buffer, shadow)."""
        old, new = self.n, self.n + m
        crossed = dict(head=new > self.cache_rows, shadow=bool(self.quant) and new > self.q_rows,
                       bits=self.bits_cap > 0 and _align(max(old, 4), 256) <= self.bits_cap < _align(max(new, 4), 256))
        if crossed["head"]:
            self.cache_rows = new + new // 2 + 64
        if self.quant:
            self._reserve(new)
        self.n = new
        return crossed

    def compact(self, m):
        self.cache_rows = m + m // 4 + 64
        if self.quant:
            self.q_rows = m + m // 4 + 64
        self.n = m

    def update(self, n2):
        if n2 > self.cache_rows:
            self.cache_rows = n2 + n2 // 4 + 64
        if self.quant:
            self._reserve(n2)
        self.n = n2
        self.poison = None

    def probe(self, kind):
        if kind in ("bits", "all"):
            npad = _align(max(self.n, 4), 256)
            if self.bits_cap < npad:
                self.bits_cap = _align(npad + npad // 4, 256)
            self.bits_seen = self.n
        if kind in ("pearson", "all"):
            self.pearson_seen = self.n
        if kind in ("dense", "all") and self.kind == "auto" and self.quant is None and self.auto_armed and \
                self.n > CAND_CAP and self.poison is None:
            self.quant, self.q_rows = "auto", self.n + 64


def keep_rows(kind, n, rng):
    """The ascending rows a compaction of `kind` keeps (at least one: a matrix of one row keeps it)."""
    if kind == "identity" or n == 1:
        return np.arange(n, dtype=np.int64)
    if kind == "but_first":
        return np.arange(1, n, dtype=np.int64)
    if kind == "but_last":
        return np.arange(n - 1, dtype=np.int64)
    if kind == "single":
        return np.array([int(rng.integers(0, n))], dtype=np.int64)
    if kind == "prefix":
        return np.arange(max(1, n // 2), dtype=np.int64)
    if kind == "suffix":
        return np.arange(n - max(1, n // 3), n, dtype=np.int64)
    frac = 2 if kind == "half" else 16
    m = max(1, n // frac)
    return np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)


def append_size(kind, caps, rng):
    if kind == "to256":
        return _align(caps.n + 1, 256) - caps.n
    if kind == "past_head":
        return caps.cache_rows - caps.n + 1
    if kind == "past_shadow":
        return caps.q_rows - caps.n + 1
    if kind == "random":
        return int(rng.integers(20, 2001))
    return int(kind)


class _Builder:
    """Grows a step list while a Caps follows it; every step records the row counts and capacities valid BEFORE its op."""

    def __init__(self, case, seed, n0):
        self.c = CASES[case]
        self.rng = np.random.default_rng([seed, self.c["id"], 11])
        self.caps = Caps(n0, self.c["shadow"])
        self.steps = []

    def add(self, op, probe, kind=None, m=None):
        caps, rng = self.caps, self.rng
        st = dict(op=op, probe=probe, kind=kind, n0=caps.n, cache_rows=caps.cache_rows, bits_cap=caps.bits_cap, q_rows=caps.q_rows,
                  quant=caps.quant, bits_seen=caps.bits_seen, pearson_seen=caps.pearson_seen, crossed=dict(head=False, bits=False, shadow=False))
        if op == "append":
            st["m"] = m if m is not None else append_size(kind, caps, rng)
            st["crossed"] = caps.append(st["m"])
        elif op in ("poison_nan", "poison_inf"):
            st["m"] = 1
            st["crossed"] = caps.append(1)
            caps.poison = (op[7:], caps.n - 1)
        elif op == "compact":
            st["keep"] = keep_rows(kind, caps.n, rng)
            if caps.poison is not None:                      # the poisoned row stays the model's to find: it travels with the rows
                pos = np.searchsorted(st["keep"], caps.poison[1])
                caps.poison = (caps.poison[0], int(pos)) if pos < st["keep"].size and st["keep"][pos] == caps.poison[1] else None
            caps.compact(int(st["keep"].size))
        elif op == "heal":
            row = caps.poison[1]
            st["keep"] = np.delete(np.arange(caps.n, dtype=np.int64), row)
            caps.compact(caps.n - 1)
            caps.poison = None
        elif op == "update":
            st["m"] = m
            caps.update(m)
        elif op == "quantize_on":
            caps.quantize(True)
        elif op == "quantize_off":
            caps.quantize(False)
        elif op not in ("set_bias", "set_mask", "set_subset"):
            raise ValueError(op)
        caps.probe(probe)
        st["n1"] = caps.n
        self.steps.append(st)


def start_rows(case, seed):
    return 290 + int(np.random.default_rng([seed, CASES[case]["id"], 5]).integers(0, 40))       # n % 256 in [34, 74)


def schedule(case, seed):
    """The step list of the GPU test: every op kind the case allows, every probe kind, and the orders the coverage conditions of
    tests/test_lifecycle_inputs.py name, in at most MAX_STEPS steps with 1 <= n <= N_MAX."""
    c = CASES[case]
    b = _Builder(case, seed, start_rows(case, seed))
    rng, add = b.rng, b.add
    add("append", "bits", "1")                                   # inside a partly packed 256-row block
    add("append", "pearson", "15")                               # pscale_done runs ahead of bits_done
    add("append", "none", "17")
    add("compact", "none", "half")                               # below what the bit and the pearson probe saw ...
    add("append", "none", "3")                                   # ... an append right behind the gather, no probe between
    add("append", "bits", "to256")
    add("append", "pearson", "16")
    add("set_bias", "dense")
    add("append", "dense", "past_head")
    add("set_mask", "dense")
    add("append", "all", "255")
    add("set_subset", "dense")
    add("append", "dense", "256")                                # crosses the bit buffer's capacity; the next bit probe regrows it
    if c["shadow"] == "explicit":
        add("append", "all", "past_shadow")
    add("append", "none", "257")
    if c["nan"]:
        add("poison_nan", "all")
        add("heal", "all")
    if c["shadow"] == "explicit":
        add("quantize_off", "dense")                             # ... right after a compaction (the heal)
        add("quantize_on", "none")
    add("update", "bits", m=7700 + int(rng.integers(0, 300)))    # larger
    add("append", "all", "random", m=CAND_CAP - b.caps.n + int(rng.integers(100, 400)))     # (builds the automatic shadow)
    if c["shadow"] == "auto":
        add("append", "dense", "past_shadow")                    # the automatic build left no room
    if c["inf"]:
        add("poison_inf", "all")
        add("heal", "all")
    if c["shadow"] == "auto":
        add("quantize_off", "dense")                             # dropping it switches the automatic build off: an explicit one follows
        add("quantize_on", "none")
    add("compact", "dense", "identity")
    add("compact", "pearson", "but_first")
    add("compact", "bits", "but_last")
    add("append", "none", "random", m=int(rng.integers(500, 2001)))
    add("compact", "all", "sixteenth")
    add("compact", "none", "prefix")
    add("compact", "all", "suffix")
    add("update", "all", m=max(8, b.caps.n * 2 // 3))            # smaller, every lazy cache warm
    add("compact", "all", "single")
    add("append", "all", "random", m=int(rng.integers(20, 300)))
    return b.steps


def pinned_schedule(name):
    """-> (case, seed, steps): the shortest schedule that still showed a library bug the random walk found.
    masked_rows_in_the_full_sort: a row mask on more than CAND_CAP rows and k = n > 2048 -- the radix sort of all scores returned
    the excluded rows by index behind the kept ones (score -inf) where every other path pads with -1 / -inf."""
    if name == "masked_rows_in_the_full_sort":
        case, seed = "f32", 3
        b = _Builder(case, seed, start_rows(case, seed))
        b.add("update", "none", m=CAND_CAP + 100)
        b.add("set_mask", "all")
        return case, seed, b.steps
    raise KeyError(name)


PINNED = ("masked_rows_in_the_full_sort",)


def random_schedule(case, seed, steps):
    """A long random walk over the same ops for the command line (no coverage promise); ends with an `all` probe."""
    c = CASES[case]
    b = _Builder(case, seed, start_rows(case, seed))
    rng = b.rng
    probes = list(PROBES)
    while len(b.steps) < steps:
        caps = b.caps
        probe = probes[int(rng.integers(0, len(probes)))] if len(b.steps) < steps - 1 else "all"
        if caps.poison is not None:
            b.add("heal" if rng.random() < 0.7 else "set_bias", probe)
            continue
        ops = ["append"] * 6 + ["compact"] * 4 + ["update", "set_bias", "set_mask", "set_subset"]
        if c["shadow"]:
            ops += ["quantize_off" if caps.quant else "quantize_on"]
        if c["nan"]:
            ops.append("poison_nan")
        if c["inf"]:
            ops.append("poison_inf")
        op = ops[int(rng.integers(0, len(ops)))]
        if op == "append":
            kinds = [k for k in APPEND_KINDS if k != "past_shadow" or caps.quant]
            kind = kinds[int(rng.integers(0, len(kinds)))]
            m = append_size(kind, caps, rng)
            if caps.n + m > N_MAX:
                op = "compact"
            else:
                b.add("append", probe, kind, m=m)
                continue
        if op == "compact":
            b.add("compact", probe, COMPACT_KINDS[int(rng.integers(0, len(COMPACT_KINDS)))])
        elif op == "update":
            b.add("update", probe, m=int(rng.integers(1, N_MAX + 1)))
        elif op in ("poison_nan", "poison_inf") and caps.n + 1 > N_MAX:
            b.add("compact", probe, "half")
        else:
            b.add(op, probe)
    return b.steps


# ---- data ----------------------------------------------------------------------------------------------------------------------------
def convert(storage, raw):
    """Incoming data -> the values the device stores, widened exactly, with the project's own host conversions: numpy's round to
    nearest even for float16, torch's on the CPU for bfloat16, to_f8 and to_i8 (hyperdb/_native.py)."""
    raw = np.asarray(raw)
    if storage == "float16":
        return raw.astype(np.float16)
    if storage == "float32":
        return raw.astype(np.float32)
    if storage == "float64":
        return raw.astype(np.float64)
    import torch
    if storage == "bfloat16":
        return torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).to(torch.bfloat16).float().numpy()
    from hyperdb._native import to_f8, to_i8
    if storage == "float8":
        return to_f8(np.ascontiguousarray(raw, dtype=np.float32)).float().numpy()
    if storage == "int8":
        return to_i8(raw).numpy().astype(np.float32)
    raise ValueError(storage)


class Data:
    """Seeded rows and the six probe queries of one (case, seed).  Rows are a common mean vector (entries of +-0.1 .. 0.3, so every row
    and every query share a dominant direction and a score is never small against |v| |q|) plus N(0, 0.1^2) noise; int8 rows are the
    integers nearest to 80 times that.  Blocks of 8+ rows carry planted rows: all zero, constant 0.25 (pearson NaN), an exact duplicate
    pair, probe query 0 itself, and a row scaled up and one scaled down (1e3 and 1e-3; float8 256 and 1/64 inside +-448; int8 4 and 1/8)."""

    def __init__(self, case, seed):
        self.c = CASES[case]
        self.storage, self.d = self.c["storage"], self.c["d"]
        self.rng = np.random.default_rng([seed, self.c["id"], 3])
        self.raw_dt = np.float64 if self.storage == "float64" else np.float32
        self.mu = self.rng.uniform(0.1, 0.3, self.d) * self.rng.choice([-1.0, 1.0], self.d)
        rawq = self.mu * self.rng.uniform(0.8, 1.2, (NQ, self.d)) + 0.1 * self.rng.standard_normal((NQ, self.d))
        self.raw_q = self._finish(rawq)
        q = convert(self.storage, self.raw_q)
        self.Q = np.ascontiguousarray(q, dtype=np.float64 if self.storage == "float64" else np.float32)

    def _finish(self, x):
        if self.storage == "int8":
            return np.clip(np.rint(80.0 * x), -127, 127).astype(np.float32)
        if self.storage == "float8":
            x = np.clip(x, -F8_MAX, F8_MAX)
        return x.astype(self.raw_dt)

    def block(self, m):
        """-> (raw rows [m, d], planted {name: row inside the block})."""
        rng = self.rng
        x = self._finish(self.mu + 0.1 * rng.standard_normal((m, self.d)))
        planted = {}
        if m >= 8:
            at = rng.choice(m, size=8, replace=False)
            up, down = {"float8": (256.0, 1.0 / 64.0), "int8": (4.0, 0.125)}.get(self.storage, (1e3, 1e-3))
            x[at[0]] = 0
            x[at[1]] = 20 if self.storage == "int8" else 0.25
            x[at[3]] = x[at[2]]
            x[at[4]] = self.raw_q[0]
            if self.storage == "int8":
                x[at[5]] = np.clip(x[at[5]] * up, -127, 127)
                x[at[6]] = np.floor(x[at[6]] * down)
            else:
                x[at[5]] = self._finish(x[at[5]].astype(np.float64) * up)
                x[at[6]] = self._finish(x[at[6]].astype(np.float64) * down)
            planted = dict(zero=int(at[0]), const=int(at[1]), dup=(int(at[2]), int(at[3])), query0=int(at[4]), up=int(at[5]), down=int(at[6]))
        return x, planted


class Model:
    """The matrix (stored values, widened), the live per-row inputs, the shadow request and the poisoned row."""

    def __init__(self, case, seed):
        self.case, self.seed, self.c = case, seed, CASES[case]
        self.storage, self.d = self.c["storage"], self.c["d"]
        self.data = Data(case, seed)
        self.rng = np.random.default_rng([seed, self.c["id"], 13])
        raw, planted = self.data.block(start_rows(case, seed))
        self.V = convert(self.storage, raw)
        self.raw = raw                       # what the last append / update handed to the index
        self.planted_at = (0, planted)       # (first row, {name: row inside the block}) of the block that came last
        self.bias = self.mask = self.rows = None
        self.quant = "initial"               # "initial" | "off" | "on": what the caller last asked of the shadow
        self.poison = None                   # (kind, row)
        self.mutated_after_input = False

    @property
    def n(self):
        return int(self.V.shape[0])

    def _drop_inputs(self):
        self.mutated_after_input = self.bias is not None or self.mask is not None
        self.bias = self.mask = self.rows = None

    def append(self, raw):
        self.raw = raw
        self.V = np.concatenate([self.V, convert(self.storage, raw)], axis=0)
        self._drop_inputs()

    def compact(self, keep):
        keep = np.asarray(keep, dtype=np.int64)
        if self.poison is not None:
            pos = np.searchsorted(keep, self.poison[1])
            self.poison = (self.poison[0], int(pos)) if pos < keep.size and keep[pos] == self.poison[1] else None
        self.V = np.ascontiguousarray(self.V[keep])
        self._drop_inputs()

    def update(self, raw):
        self.raw = raw
        self.V = convert(self.storage, raw)
        self.poison = None
        self._drop_inputs()

    def apply(self, st):
        """One op on the model -> what the index is to be given (raw rows, keep list, bias, (mask, rows))."""
        op = st["op"]
        if op == "append":
            raw, planted = self.data.block(st["m"])
            self.planted_at = (self.n, planted)
            self.append(raw)
            return raw
        if op in ("poison_nan", "poison_inf"):
            raw, _ = self.data.block(1)
            raw[0, 0 if op == "poison_inf" else int(self.rng.integers(0, self.d))] = np.inf if op == "poison_inf" else np.nan
            self.append(raw)
            self.poison = (op[7:], self.n - 1)
            return raw
        if op in ("compact", "heal"):
            self.compact(st["keep"])
            return st["keep"]
        if op == "update":
            raw, planted = self.data.block(st["m"])
            self.planted_at = (0, planted)
            self.update(raw)
            return raw
        if op == "quantize_on":
            self.quant = "on"
        elif op == "quantize_off":
            self.quant = "off"
        elif op == "set_bias":
            scale = 50.0 if self.storage == "int8" else 0.05
            self.bias = (scale * self.rng.uniform(-1.0, 1.0, self.n)).astype(np.float32)
            return self.bias
        elif op in ("set_mask", "set_subset"):
            every = 3 if op == "set_mask" else 40
            m = max(1, self.n // every)
            rows = np.sort(self.rng.choice(self.n, size=m, replace=False)).astype(np.int64)
            self.mask = np.zeros(self.n, dtype=np.uint8)
            self.mask[rows] = 1
            self.rows = rows if op == "set_subset" else None
            return self.mask, self.rows
        return None


def expected_scores(orc, V64, q, metric):
    """float64 scores of every row and where the per-metric function answers NaN: pearson on a constant row or query, jaccard on an
    empty union (the oracle writes -inf there, as the ranking does), and wherever the arithmetic itself gives NaN."""
    with np.errstate(all="ignore"):
        ref = orc.exact_scores(V64, q, metric)
    nan = np.isnan(ref)
    if metric in ("pearson_correlation", "jaccard_similarity"):
        nan |= np.isneginf(ref)
    return ref, nan


def tie_hazards(exact, k, tol, noise):
    """A top-k whose k-th and (k+1)-th exact scores differ by more than check_topk's slack (2 tol |s_k|) and by no more than twice
    the rounding noise of a correct float32 kernel could come back with the two swapped and fail check_topk for no fault of its own."""
    s = np.sort(exact[np.isfinite(exact)])[::-1]
    if k >= s.size:
        return False
    gap = s[k - 1] - s[k]
    return 2.0 * tol * abs(s[k - 1]) < gap <= 2.0 * noise


def f32_noise(metric, d, exact_k, storage):
    """4 sigma of d float32 roundings accumulated at random.  Relative to the score for dot (the rows share the query's direction:
    sum |v_i q_i| is of the size of |s|) and for euclidean / manhattan (s = 1 / (1 + x): a relative error e of the distance x moves
    s by s^2 x e < s e); absolute, against 1, for cosine and pearson, whose numerator and norms are rounded separately."""
    if metric == "hamming_distance":
        return 0.0
    if metric == "jaccard_similarity":
        return 2.0 ** -23
    u = 2.0 ** -53 if storage == "float64" else 2.0 ** -24
    size = 1.0 if metric in ("cosine_similarity", "pearson_correlation") else abs(exact_k)
    return 4.0 * np.sqrt(d) * u * size + (2.0 ** -24) * abs(exact_k)           # (... and the float32 result itself)


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------
def _upload(storage, V):
    import torch
    if storage == "bfloat16":
        return torch.from_numpy(np.ascontiguousarray(V, dtype=np.float32)).to(torch.bfloat16)
    if storage == "float8":
        from hyperdb._native import to_f8
        return to_f8(np.ascontiguousarray(V, dtype=np.float32))
    return np.ascontiguousarray(V)


def open_index(case, V, quant="initial"):
    """A GpuIndex over the stored values V with the case's options; quant: what the caller last asked of the shadow."""
    from hyperdb._native import GpuIndex
    c = CASES[case]
    ix = GpuIndex(_upload(c["storage"], V), storage="int8" if c["storage"] == "int8" else None)
    ix.set_option("subset_min_n", 0)
    ix.set_option("subset_ratio", 1)
    if c["shadow"] == "explicit":
        if c["storage"] == "bfloat16":
            ix.set_option("bf16_quant", 1)
        else:
            ix.set_option("use_mfma", 0)
            ix.set_option("use_fused", 0)
        if quant != "off":
            ix.quantize("int8")
    if c["shadow"]:
        ix.set_option("quant_min_n", 0)
        ix.set_option("plane_min_n", 0)
        if quant == "off":
            ix.quantize(None)
        elif quant == "on" and c["shadow"] == "auto":
            ix.quantize("int8")
    return ix


def _bits(x):
    """float32 values as their int32 words; every NaN as one word (which NaN a row gives depends on the NaN that was stored, and a
    float32 NaN rounded to bfloat16 on the device need not be the NaN torch makes of it on the host)."""
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    return np.where(np.isnan(x), np.int32(0x7FC00000), x.view(np.int32))


def _first_diff(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    if a.shape != b.shape:
        return f"shapes {a.shape} / {b.shape}"
    bad = np.flatnonzero(a != b)
    return int(bad[0]) if bad.size else None


class Failure(AssertionError):
    pass


class Runner:
    """One long-lived GpuIndex beside the model; step() applies an op to both and checks the probe."""

    def __init__(self, case, seed, steps):
        from hyperdb import _native
        from oracle import ranking_oracle
        self.nat, self.orc = _native, ranking_oracle
        self.case, self.seed, self.steps, self.c = case, seed, steps, CASES[case]
        self.model = Model(case, seed)
        self.caps = Caps(self.model.n, self.c["shadow"])
        self.ix = open_index(case, self.model.V)
        self.Q = self.model.data.Q
        self.counts = dict(subset=0, shadow_calls=0, plane_calls=0, bounds=0, bounds_after_mutation=0, unmasked_after_input=0)
        self.where = {}

    def close(self):
        self.ix.close()

    def fail(self, what, row=None):
        w = self.where
        raise Failure(f"(case, seed, step) = ({self.case!r}, {self.seed}, {w.get('i')}): op {w.get('op')} probe {w.get('probe')} "
                      f"metric {w.get('metric')} first differing row {row}: {what}")

    def need(self, cond, what, row=None):
        if not cond:
            self.fail(what, row)

    # -- ops -----------------------------------------------------------------------------------------
    def _payload(self, raw, stored=False):
        """Appends hand over the incoming data as it is (the index converts); a float16 update needs the stored dtype."""
        s = self.c["storage"]
        return _upload(s, convert(s, raw)) if stored else raw

    def apply(self, st):
        m, ix, op = self.model, self.ix, st["op"]
        had_input = m.bias is not None or m.mask is not None
        out = m.apply(st)
        if op in ("append", "poison_nan", "poison_inf"):
            ix.append(self._payload(out))
        elif op in ("compact", "heal"):
            ix.compact(out)
        elif op == "update":
            ix.update(self._payload(out, stored=self.c["storage"] == "float16"))
        elif op == "quantize_on":
            ix.quantize("int8")
        elif op == "quantize_off":
            ix.quantize(None)
        elif op == "set_bias":
            ix.set_bias(out)
        elif op == "set_mask":
            ix.set_row_mask(out[0])
        elif op == "set_subset":
            ix.set_row_subset(out[0], out[1])
        if op in ("append", "poison_nan", "poison_inf", "compact", "heal", "update"):
            self.need(ix._bias is None and ix._mask is None and ix._rows is None and len(ix._rows_ok) == 0,
                      "a per-row input survived the mutation on the Python side")
            self.need(ix.stat("subset_rows") == 0, "the library kept a row list across the mutation")
            self.after_input = had_input
        else:
            self.after_input = False
        self.need(ix.n == m.n == ix.stat("n"), f"n: index {ix.n}, library {ix.stat('n')}, model {m.n}")

    # -- probes --------------------------------------------------------------------------------------
    def _fresh(self):
        m = self.model
        fresh = open_index(self.case, m.V, m.quant)
        if m.bias is not None:
            fresh.set_bias(m.bias)
        if m.rows is not None:
            fresh.set_row_subset(m.mask, m.rows)
        elif m.mask is not None:
            fresh.set_row_mask(m.mask)
        return fresh

    def probe(self, st):
        m, ix, orc = self.model, self.ix, self.orc
        metrics = PROBES[st["probe"]]
        if not metrics:
            return
        M = self.nat.METRIC_IDS
        storage, n = self.c["storage"], m.n
        # (d) bookkeeping
        host = ix.host_matrix()
        self.need(host.dtype == m.V.dtype and host.shape == m.V.shape, f"host_matrix {host.dtype}{host.shape}, model {m.V.dtype}{m.V.shape}")
        same = (host == m.V) | (np.isnan(host) & np.isnan(m.V))
        self.need(bool(same.all()), "host_matrix differs from the model", row=None if same.all() else int(np.flatnonzero(~same.all(axis=1))[0]))
        has_nan = bool(np.isnan(m.V).any())
        self.need(ix.has_nan == has_nan, f"has_nan {ix.has_nan}, the model holds {'a' if has_nan else 'no'} NaN")
        inf_row = m.poison[1] if m.poison is not None and m.poison[0] == "inf" else None
        V64 = m.V.astype(np.float64)
        fresh = self._fresh()
        try:
            for metric in metrics:
                self.where["metric"] = metric
                tol = tol_of(storage, metric)
                exact = [expected_scores(orc, V64, self.Q[qi], metric) for qi in range(NQ)]
                # (a) every row against float64, (b) every row against the fresh index, bit for bit
                for qi in (0, 1):
                    got = ix.scores(self.Q[qi], M[metric]).cpu().numpy()
                    want = fresh.scores(self.Q[qi], M[metric]).cpu().numpy()
                    ref, nan = exact[qi]
                    rows = np.ones(n, dtype=bool)
                    if inf_row is not None:
                        rows[inf_row] = False
                    g = got.astype(np.float64)
                    bad = rows & (np.isnan(g) != nan)
                    self.need(not bad.any(), f"query {qi}: NaN where the float64 scores have none, or the reverse", row=int(np.flatnonzero(bad)[0]) if bad.any() else None)
                    ok = rows & ~nan
                    with np.errstate(invalid="ignore"):
                        err = np.abs(g[ok] - ref[ok])
                        out = ~(err <= tol * np.maximum(1.0, np.abs(ref[ok])))
                    if out.any():
                        r = int(np.flatnonzero(ok)[np.flatnonzero(out)[0]])
                        self.fail(f"query {qi}: score {float(g[r])!r}, float64 {float(ref[r])!r}, tolerance {tol}", row=r)
                    self.need(np.array_equal(_bits(got), _bits(want)), f"query {qi}: scores() differs from the fresh index",
                              row=_first_diff(_bits(got), _bits(want)))
                # (c) top-k
                self._topk(metric, fresh, exact, tol, inf_row, has_nan)
            if "cosine_similarity" in metrics and not has_nan:
                self._shadow(fresh, metrics)
        finally:
            fresh.close()
        self.where["metric"] = None

    def _topk(self, metric, fresh, exact, tol, inf_row, has_nan):
        m, ix, orc = self.model, self.ix, self.orc
        mid, n = self.nat.METRIC_IDS[metric], m.n
        if has_nan:                                          # the entry points raise on has_nan (checked above) before any top-k call:
            return                                           # ranking resumes with the heal
        if m.bias is not None and tol == 0.0:
            tol = 1e-5                                       # an integer score plus a float32 bias: a float32 sum
        part = np.arange(n) if m.mask is None else np.flatnonzero(m.mask)
        for nq in (1, 3, NQ):
            for k in sorted({1, min(100, n), n}):
                gi, gs = ix.topk(self.Q[:nq], k, mid)
                if m.rows is not None:
                    self.counts["subset"] += ix.stat("subset")
                fi, fs = fresh.topk(self.Q[:nq], k, mid)
                self.need(np.array_equal(gi, fi), f"nq={nq} k={k}: indices differ from the fresh index", row=_first_diff(gi, fi))
                self.need(np.array_equal(_bits(gs), _bits(fs)), f"nq={nq} k={k}: score bits differ from the fresh index", row=_first_diff(_bits(gs), _bits(fs)))
                kk = min(k, part.size)
                for qi in range(nq):
                    idx, sc = gi[qi], gs[qi]
                    self.need((idx[kk:] == -1).all() and np.isneginf(sc[kk:]).all(), f"nq={nq} k={k} query {qi}: entries past the {kk} rows that take part")
                    idx, sc = idx[:kk], sc[:kk]
                    rows = part
                    ref = exact[qi][0] if m.bias is None else exact[qi][0] + m.bias.astype(np.float64)
                    if inf_row is not None:                  # the poisoned row is left out of the comparison, wherever it landed
                        sel = idx != inf_row
                        idx, sc, rows = idx[sel], sc[sel], rows[rows != inf_row]
                    pos = np.searchsorted(rows, idx)
                    self.need(bool((pos < rows.size).all()) and bool((rows[np.minimum(pos, rows.size - 1)] == idx).all()),
                              f"nq={nq} k={k} query {qi}: a returned row does not take part")
                    try:
                        orc.check_topk(pos, sc, np.empty((rows.size, 1), dtype=np.float32), self.Q[qi], metric, idx.size, tol=tol, exact=ref[rows])
                    except AssertionError as e:
                        self.fail(f"nq={nq} k={k} query {qi}: {e}")
        if self.after_input and not has_nan:
            self.counts["unmasked_after_input"] += 1         # (check_topk above ran over all rows without a bias: the model dropped them)

    def _shadow(self, fresh, metrics):
        """One query, top 100: the candidate and survivor counts of the shadow path equal the fresh index's; with a plane on both
        sides the per-row bounds of the int8 pass and of the plane are bit-equal over all rows."""
        m, ix = self.model, self.ix
        M = self.nat.METRIC_IDS
        d, n = self.c["d"], m.n
        k = min(100, n)
        stats = []
        self.where["metric"] = "cosine_similarity"
        for h in (ix, fresh):
            h.topk_device(self.Q[:1], k, M["cosine_similarity"])
            stats.append({s: h.stat(s) for s in ("quant", "plane", "quant_cands", "plane_survivors")})
        self.need(stats[0] == stats[1], f"one-query top-{k}: {stats[0]} on the index, {stats[1]} on the fresh one")
        self.counts["shadow_calls"] += stats[0]["quant"]
        self.counts["plane_calls"] += stats[0]["plane"]
        caps = self.caps
        rowb = 20 * ((_align(d, 16) + 31) // 32) + 16
        want = n * rowb if caps.quant else 0
        self.need(ix.stat("plane_bytes") == want, f"plane_bytes {ix.stat('plane_bytes')}, expected {want}")
        self.need(ix.stat("quant_bytes") == (n * (_align(d, 16) + 12) if caps.quant else 0), f"quant_bytes {ix.stat('quant_bytes')}")
        if ix.stat("plane_bytes") and fresh.stat("plane_bytes"):
            for metric in ("dot_product", "cosine_similarity"):
                self.where["metric"] = metric
                a, b = ix.quant_bounds(self.Q[0], M[metric]), fresh.quant_bounds(self.Q[0], M[metric])
                for name, x, y in (("int8 bound", a[0], b[0]), ("plane bound", a[1], b[1])):
                    self.need(np.array_equal(_bits(x), _bits(y)), f"{metric}: {name} differs from the fresh index", row=_first_diff(_bits(x), _bits(y)))
            self.counts["bounds"] += 1
            self.counts["bounds_after_mutation"] += self.mutations > 0

    def run(self, upto=None, log=None):
        self.mutations = 0
        self.after_input = False
        for i, st in enumerate(self.steps if upto is None else self.steps[:upto + 1]):
            self.where = dict(i=i, op=st["op"] + (f"({st['kind'] or st.get('m')})" if st["op"] in ("append", "compact", "update") else ""),
                              probe=st["probe"], metric=None)
            try:
                self.apply(st)
                self.mutations += st["op"] in ("append", "poison_nan", "poison_inf", "compact", "heal", "update")
                # the row-count simulation follows, so the probe knows whether a shadow exists
                self._follow(st)
                self.probe(st)
            except Failure:
                raise
            except Exception as e:                           # a library error is a finding of this step too
                self.fail(f"{type(e).__name__}: {e}")
            if log:
                log(f"step {i:3d} {self.where['op']:<22} probe {st['probe']:<8} n = {self.model.n}")
        return self.counts

    def _follow(self, st):
        caps, op = self.caps, st["op"]
        if op in ("append", "poison_nan", "poison_inf"):
            caps.append(st.get("m", 1))
            if op != "append":
                caps.poison = (op[7:], caps.n - 1)
        elif op in ("compact", "heal"):
            caps.compact(int(st["keep"].size))
            caps.poison = self.model.poison
        elif op == "update":
            caps.update(st["m"])
        elif op == "quantize_on":
            caps.quantize(True)
        elif op == "quantize_off":
            caps.quantize(False)
        caps.probe(st["probe"])


def run(case, seed, steps=None, upto=None, log=None):
    """Apply a schedule (default: schedule(case, seed)) to the model and one GpuIndex; raises Failure at the first step that misses."""
    r = Runner(case, seed, schedule(case, seed) if steps is None else steps)
    try:
        return r.run(upto=upto, log=log)
    finally:
        r.close()


def replay(case, seed, step, steps=None):
    return run(case, seed, steps=steps, upto=step, log=print)


if __name__ == "__main__":
    n_steps, seed = int(sys.argv[1]), int(sys.argv[2])
    bad = 0
    for case in ([sys.argv[3]] if len(sys.argv) > 3 else list(CASES)):
        try:
            counts = run(case, seed, steps=random_schedule(case, seed, n_steps))
            print(f"{case}: {n_steps} steps ok {counts}", flush=True)
        except Failure as e:
            bad += 1
            print(f"FAIL {e}", flush=True)
    sys.exit(1 if bad else 0)
