"""CPU model of the plane pass on its hot blocks (hdb_quant.hip, "The 5-bit plane": the hot block; hdb_caps.h, hdb_plane_*): per
16-row tile and metric flavour the scale of a row rounded up to bfloat16, the residual norm as the byte ceil(2 R), and the tile's
maxima E*, T*, F*.  Every float32 operation of the two kernels is done in numpy float32, and hi5 >= hi must hold for MODE 1's hi on

  random codes and the adversarial rows of tests/test_quant_plane_model.py (every residual -4 or +3 with the query's signs aligned,
  all +-127, a zero row), and
  heterogeneous tiles: norms from 1e-4 to 1e4 inside one tile, all-zero rows and rows of +-65504, mixed into the other rows' tiles,

for both metrics, with and without bias, d in {16, 40, 384, 512}.  The last tile is ragged: its missing rows take no part in the maxima.
No GPU."""
import numpy as np
import pytest

from test_quant_plane_model import DIMS, F, _hi_int8, _plane, _queries, _rows, _sum_cq_u, _up

U32 = np.uint32


def _bf16_up(k):
    """hdb_plane_k_encode: the smallest bfloat16 at or above the non-negative float64 k, as its 16 bits."""
    k = np.asarray(k, np.float64)
    h = (k.astype(F).view(U32) >> 16).astype(U32)
    below = (h << 16).view(F).astype(np.float64) < k
    return (h + below.astype(U32)).astype(U32)


def _k_hi(code):
    return (code.astype(U32) << 16).view(F)


def _k_lo(k_hi):
    ok = (k_hi >= F(2.0 ** -126)) & np.isfinite(k_hi)
    return np.where(ok, (k_hi * F(1 - 2.0 ** -7)).astype(F), F(0)).astype(F)


def _rc(ss):
    """hdb_plane_rc_encode: the smallest integer rc with rc^2 >= 4 ss."""
    rc = np.ceil(2.0 * np.sqrt(ss.astype(np.float64))).astype(np.int64)
    rc += (rc * rc < 4 * ss)
    rc -= ((rc - 1) * (rc - 1) >= 4 * ss) & (rc > 0)
    assert (rc * rc >= 4 * ss).all() and rc.max() <= 182
    return rc


def _upv(x):
    return np.array([_up(float(v)) for v in np.asarray(x, np.float64)], F)


def _tile_max(x, n):
    """the maximum over each 16-row tile's rows (rows below n only), repeated for every row of the tile"""
    pad = (-n) % 16
    t = np.concatenate([x, np.zeros(pad, x.dtype)]).reshape(-1, 16).max(axis=1)
    return np.repeat(t, 16)[:n]


def _blocks(s_r, E_r, T_r, invn, ss, d, cosine):
    """What hdb_quant_plane_rows_kernel leaves for one flavour: k_hi [n], R [n], and E*, T*, F* of each row's tile."""
    n = s_r.size
    w = invn.astype(np.float64) if cosine else np.ones(n)
    k_hi = _k_hi(_bf16_up(s_r.astype(np.float64) * w))
    R = (F(0.5) * _rc(ss).astype(F)).astype(F)
    assert (R.astype(np.float64) ** 2 >= ss).all()
    absmin = 2.0 ** -100 * (d + 8)
    Es = _tile_max(_upv(E_r.astype(np.float64) * w), n)
    Ts = _tile_max(_upv(T_r.astype(np.float64) * w), n)
    Fs = _tile_max(_upv(absmin * w * (1 + 2.0 ** -40)), n)
    return k_hi, R, Es, Ts, Fs


def _hi5(C5, q_cn, q_s, N_q, D_q, blk, cosine, q_inv, bias):
    """Pass 1's upper bound on the hot block, operation by operation in float32."""
    k_hi, R, Es, Ts, Fs = blk
    fc = C5.astype(F)
    Uf = (q_cn * R).astype(F)
    ch = (fc + Uf).astype(F)
    cl = (fc - Uf).astype(F)
    ch = (ch + ((np.abs(ch) * F(2.0 ** -20)).astype(F) + F(1))).astype(F)
    cl = (cl - ((np.abs(cl) * F(2.0 ** -20)).astype(F) + F(1))).astype(F)
    k_up = (q_s * k_hi).astype(F)
    k_dn = (q_s * _k_lo(k_hi)).astype(F)
    k_up = (k_up + (k_up * F(2.0 ** -20)).astype(F)).astype(F)
    k_dn = (k_dn - (k_dn * F(2.0 ** -20)).astype(F)).astype(F)
    A5 = (np.where(ch >= 0, k_up, k_dn) * ch).astype(F)
    Al = (np.where(cl >= 0, k_dn, k_up) * cl).astype(F)
    Amax = np.maximum(np.abs(A5), np.abs(Al))
    c0 = (((N_q * Es).astype(F) + (D_q * Ts).astype(F)).astype(F) * F(1 + 2.0 ** -10)).astype(F)
    B5 = ((c0 + np.abs(A5) * F(2.0 ** -10)).astype(F) + Fs).astype(F)
    Bmax = ((c0 + Amax * F(2.0 ** -10)).astype(F) + Fs).astype(F)
    Mx = (Amax + Bmax).astype(F)
    X = ((A5 + B5).astype(F) + ((Mx * F(2.0 ** -18)).astype(F) + F(1e-30))).astype(F)
    mM = (Mx * F(1 + 2.0 ** -17)).astype(F)
    if cosine:
        X = (X * q_inv).astype(F)
        mM = (mM * q_inv).astype(F)
    Z = (mM + np.abs(bias if bias is not None else F(0))).astype(F)
    h = X if bias is None else (X + bias).astype(F)
    return (h + ((Z * F(2.0 ** -18)).astype(F) + F(4e-30))).astype(F), ch, cl, A5, Al


def _matrix(rng, d, P):
    """Codes and scales: the random and adversarial rows of the parent model at ordinary scales, then rows whose norms run from 1e-4
    to 1e4, zero rows and rows of +-65504 -- shuffled, so that the extreme rows share tiles with ordinary ones."""
    codes, first = _rows(rng, d, P, 200)
    n0 = codes.shape[0]
    s0 = (rng.random(n0) * 0.05 + 1e-3).astype(F)
    s0[-1] = F(0)                                    # the zero row of _rows
    m = 96
    wild = np.zeros((m + 12, P), np.int8)
    wild[:m, :d] = np.clip(np.rint(rng.standard_normal((m, d)) * 36), -127, 127)
    wild[:m, 0] = 127
    norms = 10.0 ** rng.uniform(-4, 4, size=m)
    sw = (norms / np.sqrt((wild[:m].astype(np.float64) ** 2).sum(axis=1))).astype(F)
    wild[m + 6:m + 9, :d] = 127; wild[m + 9:, :d] = -127       # +-65504 in every element; rows m .. m + 5 stay zero
    sw = np.concatenate([sw, np.zeros(6, F), np.full(6, F(65504.0) / F(127.0), F)])
    codes = np.concatenate([codes, wild]); s_r = np.concatenate([s0, sw])
    order = rng.permutation(codes.shape[0])
    # the three tight adversarial rows keep their numbers' meaning for _queries: return where they went
    where = np.argsort(order)
    return codes[order], s_r[order], [int(where[first + i]) for i in range(3)]


@pytest.mark.parametrize("d", DIMS)
def test_hi5_on_the_hot_block_bounds_mode1(d):
    rng = np.random.default_rng(1000 + d)
    P = (d + 15) // 16 * 16
    codes, s_r, tight = _matrix(rng, d, P)
    n = codes.shape[0]
    assert n % 16 != 0, "the last tile is ragged"
    nib, bit, _, rho = _plane(codes, d)
    ss = (rho.astype(np.int64) ** 2).sum(axis=1)
    c64 = codes.astype(np.int64)
    cn = np.sqrt((c64 ** 2).sum(axis=1).astype(np.float64))
    T_r = _upv(s_r.astype(np.float64) * cn)
    E_r = (s_r * F(0.3 * np.sqrt(d))).astype(F)
    norm = s_r.astype(np.float64) * cn
    invn = np.where(norm > 0, 1.0 / np.maximum(norm, 1e-300), 1.0).astype(F)       # (hdb_rownorm_kernel: 1 for a zero row)
    per_tile = norm[: n // 16 * 16].reshape(-1, 16)
    assert (per_tile.max(axis=1) / np.maximum(per_tile.min(axis=1), 1e-30)).max() > 1e6, "no heterogeneous tile"
    absmin = F(2.0 ** -100 * (d + 8))
    blocks = {cos: _blocks(s_r, E_r, T_r, invn, ss, d, cos) for cos in (False, True)}
    rho_q = np.stack([rho[t] for t in tight])                                      # _queries aligns its signs with these three rows
    for qc in _queries(rng, d, codes, rho_q, 0):
        C = c64[:, :d] @ qc
        C5 = 8 * _sum_cq_u(nib, bit, qc) - 124 * int(qc.sum())
        q_cn = _up(np.sqrt(float((qc ** 2).sum())))
        for s_q in (F(0.02), F(3e-5), F(40.0)):
            k = (s_q * s_r).astype(F)
            N_q = _up(float(s_q) * np.sqrt(float((qc ** 2).sum())) * 1.001)
            D_q = _up(float(s_q) * 0.29 * np.sqrt(d))
            c0 = (((N_q * E_r).astype(F) + (D_q * T_r).astype(F)).astype(F) * F(1 + 2.0 ** -10)).astype(F)
            for cosine in (False, True):
                q_inv = F(1.0 / max(float(N_q), 1e-6)) if cosine else F(1)
                scale = 1.0 if cosine else float(np.abs(k).max()) * 1e4
                for bias in (None, (rng.random(n) * 0.05 * scale).astype(F), (-rng.random(n) * 5 * scale).astype(F)):
                    hi = _hi_int8(C, k, c0, absmin, cosine, invn, q_inv, bias)
                    hi5, ch, cl, A5, Al = _hi5(C5, q_cn, s_q, N_q, D_q, blocks[cosine], cosine, q_inv, bias)
                    assert (ch.astype(np.float64) >= C).all() and (cl.astype(np.float64) <= C).all()
                    # the two sides of k fl(C), in the flavour's own scaling
                    A = (k * C.astype(F)).astype(F).astype(np.float64) * (invn.astype(np.float64) if cosine else 1.0)
                    assert (A5 >= A).all() and (Al <= A).all(), f"d={d} cosine={cosine} s_q={s_q}: k C outside [Al, A5]"
                    assert np.isfinite(hi5).all(), f"d={d} cosine={cosine} s_q={s_q}: hi5 not finite"
                    bad = np.flatnonzero(~(hi5 >= hi))
                    assert bad.size == 0, f"d={d} cosine={cosine} s_q={s_q} bias={bias is not None}: hi5 < hi at rows {bad[:8]}"
