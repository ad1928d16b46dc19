"""The plane pass with its query words read from LDS and its grid from the plan (hdb_quant_plane_scan_kernel, hdb_quant.hip;
hdb_quant_plane_blocks, hdb_caps.h).  The decode is the same integer arithmetic on the same operands and the keep decision is per
row, so no grid may change anything: indices, score bits and the candidate count of a call behind the plane are those of the call
with use_plane = 0 and the answers those of the call without the shadow and of exact=True; plane_survivors is one number per shape
and query whatever the grid; plane_blocks is what the rule says (plane_blocks of tests/test_plane_grid_plan.py, the table read from
the header).

Widths: every J = ceil(U / 4) and the unit counts that are no multiple of 4 -- d = 32 (U = 1), 96 (3), 160 (5), 256 (8), 300 (10),
384 (12), 416 (13), 512 (16).  The automatic shadow exists where the matrix cores answer a one-query call (the multiples of 128 here:
256, 384, 512); the explicit one everywhere.  Sizes: n = 20 011 (ragged last tile of 11 rows), n = 8 217 (the ragged tile of 9 rows at the
smallest size the shadow path takes with room for a sample) and n = 4 099.  A matrix of up to cand_cap = 8192 rows takes no shadow
path at all (plan_topk: small), so at n = 4 099 the settings must simply change nothing -- plane_blocks and plane_survivors are 0 for
every one of them and the three answers agree; the kernel itself runs at that size in the bound check below.
Grid settings: plane_wg_per_cu in {1, 4, the table's value, 8} x max_blocks in {1, 3, 0}.

The drain case (d = 384, max_blocks = 1: four waves walk everything) plants 200 scaled copies of the query in consecutive rows of
tiles the sample did not take and one winner a hundred steps later in the share of the wave that took the first copies: that wave
drains several full tiles of 16 survivors and then goes on streaming.  The path returns at most 128 rows a call, so the copies
come back in two calls: the winner and the 127 largest copies, then -- those 127 masked -- the winner and the other 73.
"""
import numpy as np
import pytest

from hyperdb import _native
from test_plane_grid_plan import plane_blocks, wg_table
from test_plane_skip import _bits, _index, _matrix, _raw, _torch, sample_plan
from test_plane_skip_plan import tile_index

M = _native.METRIC_IDS
METRICS = ("dot_product", "cosine_similarity")
WIDTHS = (32, 96, 160, 256, 300, 384, 416, 512)
SIZES = (20011, 8217, 4099)
MAX_BLOCKS = (1, 3, 0)


def _units(d):
    return (((d + 15) // 16) * 16 + 31) // 32


def _j(d):
    return (_units(d) + 3) // 4


def _cus():
    return int(_torch().cuda.get_device_properties(0).multi_processor_count)


def _settings(d):
    return [(wg, mb) for wg in sorted({1, 4, wg_table()[_j(d) - 1], 8}) for mb in MAX_BLOCKS]


def _want_blocks(n, d, wg, mb, cus):
    s_tiles = sample_plan(n, d)[0]
    return plane_blocks((n + 15) // 16 - s_tiles, wg, cus, mb)


CASES = [(n, d, fl) for d in WIDTHS for n in SIZES for fl in ("explicit", "auto") if not (fl == "auto" and d % 128)]


def test_the_widths_cover_every_j_and_odd_unit_counts():
    assert [_units(d) for d in WIDTHS] == [1, 3, 5, 8, 10, 12, 13, 16]
    assert sorted({_j(d) for d in WIDTHS}) == [1, 2, 3, 4]
    assert len(wg_table()) == 4 and all(1 <= w <= 8 for w in wg_table())


@pytest.mark.gpu
@pytest.mark.parametrize("n,d,flavour", CASES, ids=[f"n{n}-d{d}-{fl}" for n, d, fl in CASES])
def test_no_grid_changes_anything(n, d, flavour):
    ix = _index(_matrix(n, d, seed=5 * n + d), flavour)
    cus = _cus()
    try:
        takes = n > ix.stat("cand_cap")                  # (up to cand_cap rows: no shadow path, see the module's docstring)
        for mi, metric in enumerate(METRICS):
            Q = np.random.default_rng(n + 3 * d + mi).standard_normal((1, d)).astype(np.float32)
            what = f"n={n} d={d} {flavour} {metric}"
            ix.set_option("use_plane", 0)
            off = _raw(ix, Q, 100, metric)
            assert ix.stat("plane") == 0 and ix.stat("plane_blocks") == 0 and ix.stat("quant") == (1 if takes else 0), what
            cands_off = ix.stat("quant_cands")
            ix.set_option("use_plane", 1)
            ix.set_option("use_quant", 0)
            ref = _raw(ix, Q, 100, metric)
            assert ix.stat("quant") == 0 and ix.stat("plane_blocks") == 0, what
            ix.set_option("use_quant", 1)
            ex_i, ex_s, ex_st = ix.topk_device(Q, 100, M[metric], exact=True)
            ex = (ex_i.cpu().numpy(), _bits(ex_s.cpu().numpy()), ex_st.cpu().numpy())
            assert (off[2] == 0).all() and (ref[2] == 0).all() and (ex[2] == 0).all(), f"{what}: status {off[2]} / {ref[2]} / {ex[2]}"
            survivors = set()
            for wg, mb in _settings(d):
                ix.set_option("plane_wg_per_cu", wg)
                ix.set_option("max_blocks", mb)
                on = _raw(ix, Q, 100, metric)
                blocks, surv, cands = ix.stat("plane_blocks"), ix.stat("plane_survivors"), ix.stat("quant_cands")
                where = f"{what} plane_wg_per_cu={wg} max_blocks={mb}"
                print(f"{where}: {blocks} workgroups, {surv} survivors, {cands} candidates (plane off: {cands_off})")
                assert ix.stat("plane") == (1 if takes else 0) and ix.stat("quant") == (1 if takes else 0), f"{where}: the path"
                assert blocks == (_want_blocks(n, d, wg, mb, cus) if takes else 0), f"{where}: {blocks} workgroups"
                assert cands == cands_off, f"{where}: {cands} candidates, {cands_off} with use_plane = 0"
                assert surv >= cands or not takes, f"{where}: {surv} survivors, {cands} candidates"
                survivors.add(surv)
                for a, b, c, e in zip(on, off, ref, ex):
                    assert np.array_equal(a, b), f"{where}: differs from use_plane = 0"
                    assert np.array_equal(a, c), f"{where}: differs from the call without the shadow"
                    assert np.array_equal(a, e), f"{where}: differs from exact=True"
            ix.set_option("max_blocks", 0)
            # the table's own setting
            ix.set_option("plane_wg_per_cu", 0)
            on = _raw(ix, Q, 100, metric)
            assert ix.stat("plane_blocks") == (_want_blocks(n, d, wg_table()[_j(d) - 1], 0, cus) if takes else 0), what
            survivors.add(ix.stat("plane_survivors"))
            for a, b in zip(on, off):
                assert np.array_equal(a, b), f"{what}: the default grid differs from use_plane = 0"
            assert len(survivors) == 1, f"{what}: plane_survivors {sorted(survivors)} over the grid settings"
            assert takes or survivors == {0}
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flavour", ("auto", "explicit"))
def test_one_wave_drains_several_times_and_streams_on(flavour):
    torch = _torch()
    n, d, ncopy = 20011, 384, 200
    s_tiles, stride = sample_plan(n, d)
    sampled = {tile_index(w, stride) for w in range(s_tiles)}
    walked = [t for t in range((n + 15) // 16) if t not in sampled]      # position tp of the walk is walked[tp] (hdb_plane_skip_tile)
    # one workgroup: wave w takes positions 8 i + 2 w and 8 i + 2 w + 1.  The copies fill the rows of positions 80 .. 92 (wave 0 takes
    # four of those tiles: 64 copies, four full drains), the winner sits in wave 0's pair a hundred steps later
    p0 = 80
    rows = np.concatenate([np.arange(16) + 16 * walked[p0 + i] for i in range(13)])[:ncopy]
    assert all(b - a == 1 or (a // 16 + 1) in sampled for a, b in zip(rows[:-1], rows[1:])), "consecutive rows, but for a sampled tile between"
    winner = 16 * walked[p0 + 8 * 100] + 5
    assert winner < n and winner // 16 - rows[-1] // 16 > 100
    V = _matrix(n, d, seed=11)
    q = np.random.default_rng(11).standard_normal((1, d)).astype(np.float32)
    scales = np.linspace(0.9, 0.5, ncopy).astype(np.float32)          # distinct dot products, 0.2 % of |q|^2 apart; Gaussian rows reach a third of the smallest
    qt = torch.from_numpy(q).to("cuda")
    V[torch.from_numpy(rows).to("cuda")] = (torch.from_numpy(scales).to("cuda")[:, None] * qt).to(torch.float16)
    V[winner] = (1.5 * qt[0]).to(torch.float16)
    ix = _index(V, flavour)
    try:
        ix.set_option("max_blocks", 1)
        for wg in (0, 8):
            ix.set_option("plane_wg_per_cu", wg)
            ix.set_row_mask(None)
            on = _raw(ix, q, 128, "dot_product")
            assert ix.stat("plane") == 1 and ix.stat("plane_blocks") == 1
            surv, cands = ix.stat("plane_survivors"), ix.stat("quant_cands")
            print(f"drain {flavour} plane_wg_per_cu={wg}: {surv} survivors, {cands} candidates")
            assert (on[2] == 0).all() and surv >= cands >= ncopy + 1
            assert on[0][0].tolist() == [winner] + rows[:127].tolist(), "the winner, then the copies by their scale"
            ix.set_option("use_plane", 0)
            off = _raw(ix, q, 128, "dot_product")
            ix.set_option("use_plane", 1)
            assert ix.stat("quant_cands") == cands
            for a, b in zip(on, off):
                assert np.array_equal(a, b)
            mask = torch.ones(n, dtype=torch.uint8, device="cuda")
            mask[torch.from_numpy(rows[:127]).to("cuda")] = 0
            ix.set_row_mask(mask)
            rest = _raw(ix, q, 128, "dot_product")
            assert ix.stat("plane") == 1 and (rest[2] == 0).all()
            assert rest[0][0][:74].tolist() == [winner] + rows[127:].tolist(), "the winner and the other 73 copies"
    finally:
        ix.close()


@pytest.mark.gpu
@pytest.mark.parametrize("d", (160, 300, 384, 512))
def test_coarse_bound_covers_the_fine_one(d):
    """hdb_debug_quant_bounds: hi5 >= hi elementwise, and hi5 is finite on finite rows (n = 4 099: a ragged tile of 3 rows)"""
    for n in (20011, 4099):
        ix = _index(_matrix(n, d, seed=n + d), "explicit")
        try:
            for mi, metric in enumerate(METRICS):
                q = np.random.default_rng(d + mi).standard_normal(d).astype(np.float32)
                hi, hi5 = ix.quant_bounds(q, M[metric])
                assert hi.shape == (n,) and hi5.shape == (n,)
                assert np.isfinite(hi).all() and np.isfinite(hi5).all(), f"n={n} d={d} {metric}: a bound is not finite"
                assert (hi5 >= hi).all(), f"n={n} d={d} {metric}: hi5 < hi at rows {np.flatnonzero(hi5 < hi)[:8]}"
        finally:
            ix.close()
