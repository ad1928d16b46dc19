"""CPU model of the 5-bit plane of the int8 shadow (hdb_quant.hip, "The 5-bit plane"): the packing, the integer bound
C5 - U <= C <= C5 + U and hi5 >= hi, with every float32 operation of the two kernels done in numpy float32.

No GPU: the layout and the bound are plain arithmetic.  The adversarial rows are the ones that make the Cauchy-Schwarz step tight
(every residual -4 or +3 with the query's signs aligned), rows of all +-127, zero rows and a query with one non-zero element.
"""
import numpy as np
import pytest

F = np.float32
DIMS = (16, 40, 384, 512)


def _up(x):
    """float32 >= the float64 x (hq_up)."""
    f = F(x)
    return np.nextafter(f, F(np.inf)) if float(f) < x else f


def _plane(codes, d):
    """codes [n][P] int8 -> nibble words [n][U][4], bit words [n][U], R [n] as hdb_quant_plane_rows_kernel packs them."""
    n, P = codes.shape
    U = (P + 31) // 32
    c = np.zeros((n, U * 32), np.int64)
    c[:, :P] = codes
    h = c >> 3                                       # arithmetic shift
    u5 = h + 16
    rho = c - (8 * h + 4)
    assert u5.min() >= 0 and u5.max() <= 31 and rho.min() >= -4 and rho.max() <= 3
    nib = np.zeros((n, U, 4), np.uint32)
    bit = np.zeros((n, U), np.uint32)
    for e in range(32):
        w, b = e // 4, e % 4                         # query-aligned word w of the unit, byte b
        col = u5.reshape(n, U, 32)[:, :, e]
        nib[:, :, w >> 1] |= ((col >> 1) << (8 * b + 4 * (w & 1))).astype(np.uint32)
        bit |= ((col & 1) << (8 * b + w)).astype(np.uint32)
    ss = (rho[:, :d] ** 2).sum(axis=1)
    R = (np.sqrt(ss.astype(F)) * F(1 + 2.0 ** -20)).astype(F)
    assert (R.astype(np.float64) ** 2 >= ss).all()
    return nib, bit, R, rho[:, :d]


def _sum_cq_u(nib, bit, qcodes):
    """sum_j c_qj u_rj the way pass 1 decodes it: masks and shifts on the packed words, byte-wise dot products with the query words."""
    n, U, _ = nib.shape
    q = np.zeros(U * 32, np.int64)
    q[:qcodes.size] = qcodes
    q = q.reshape(U, 8, 4)                           # [unit][query word][byte]
    S = np.zeros(n, np.int64)
    for i in range(4):
        w = nib[:, :, i]
        lo = ((w << 1) & 0x1E1E1E1E) | ((bit >> (2 * i)) & 0x01010101)
        hi = ((w >> 3) & 0x1E1E1E1E) | ((bit >> (2 * i + 1)) & 0x01010101)
        for b in range(4):
            S += (((lo >> (8 * b)) & 0xFF).astype(np.int64) * q[None, :, 2 * i, b]).sum(axis=1)
            S += (((hi >> (8 * b)) & 0xFF).astype(np.int64) * q[None, :, 2 * i + 1, b]).sum(axis=1)
    return S


def _hi_int8(C, k, c0, absmin, cosine, invn, q_inv, bias):
    """MODE 1's upper bound, operation by operation in float32."""
    A = (k * C.astype(F)).astype(F)
    B = ((c0 + np.abs(A) * F(2.0 ** -10)).astype(F) + absmin).astype(F)
    hi = (A + B).astype(F)
    if cosine:
        hi = ((hi * invn).astype(F) * q_inv).astype(F)
    if bias is not None:
        hi = (hi + bias).astype(F)
    return (hi + (np.abs(hi) * F(2.0 ** -20)).astype(F) + F(1e-30)).astype(F)


def _hi5(C5, Uf, k, c0, absmin, cosine, invn, q_inv, bias):
    """Pass 1's upper bound, operation by operation in float32."""
    fc = C5.astype(F)
    ch = (fc + Uf).astype(F)
    cl = (fc - Uf).astype(F)
    ch = (ch + ((np.abs(ch) * F(2.0 ** -20)).astype(F) + F(1))).astype(F)
    cl = (cl - ((np.abs(cl) * F(2.0 ** -20)).astype(F) + F(1))).astype(F)
    A5, Al = (k * ch).astype(F), (k * cl).astype(F)
    Amax = np.maximum(np.abs(A5), np.abs(Al))
    B5 = ((c0 + np.abs(A5) * F(2.0 ** -10)).astype(F) + absmin).astype(F)
    Bmax = ((c0 + Amax * F(2.0 ** -10)).astype(F) + absmin).astype(F)
    Mx = (Amax + Bmax).astype(F)
    X = ((A5 + B5).astype(F) + ((Mx * F(2.0 ** -18)).astype(F) + F(1e-30))).astype(F)
    mM = (Mx * F(1 + 2.0 ** -17)).astype(F)
    if cosine:
        X = ((X * invn).astype(F) * q_inv).astype(F)
        mM = ((mM * invn).astype(F) * q_inv).astype(F)
    Z = (mM + np.abs(bias if bias is not None else F(0))).astype(F)
    h = X if bias is None else (X + bias).astype(F)
    return (h + ((Z * F(2.0 ** -18)).astype(F) + F(4e-30))).astype(F), ch, cl


def _rows(rng, d, P, n_random):
    """Random codes plus the adversarial rows; returns codes [n][P] (zero past d) and the index of the first adversarial row."""
    rows = [rng.integers(-127, 128, size=(n_random, d))]
    rows.append(np.clip(np.rint(rng.standard_normal((n_random, d)) * 36), -127, 127))       # what Gaussian rows quantize to
    first = 2 * n_random
    h = rng.integers(-15, 15, size=(4, d))
    rows.append(8 * h[0:1])                          # every residual -4
    rows.append(8 * h[1:2] + 7)                      # every residual +3
    mix = rng.integers(0, 2, size=(1, d))
    rows.append(8 * h[2:3] + 7 * mix)                # -4 and +3 mixed
    rows.append(np.full((1, d), 127)); rows.append(np.full((1, d), -127))
    rows.append(np.where(rng.integers(0, 2, size=(1, d)) == 1, 127, -127))
    rows.append(np.zeros((1, d)))
    codes = np.zeros((sum(r.shape[0] for r in rows), P), np.int8)
    codes[:, :d] = np.concatenate(rows).astype(np.int8)
    return codes, first


def _queries(rng, d, codes, rho, first):
    """Random queries, the sign-aligned ones for the adversarial rows, +-127 everywhere, and one non-zero element."""
    qs = [rng.integers(-127, 128, size=d), np.clip(np.rint(rng.standard_normal(d) * 36), -127, 127).astype(np.int64)]
    for r in range(first, first + 3):
        s = np.sign(rho[r]).astype(np.int64)
        qs.append(127 * s)                           # c_q proportional to sign(rho): sum c_q rho = 127 sum |rho|
        qs.append(-127 * s)
        qs.append(np.abs(rho[r]) * 31 * s)           # c_q proportional to rho itself: equality in Cauchy-Schwarz
    qs.append(np.full(d, 127)); qs.append(np.full(d, -127))
    one = np.zeros(d, np.int64); one[d // 3] = -127
    qs.append(one)
    qs.append(np.zeros(d, np.int64))
    return [np.asarray(q, np.int64) for q in qs]


@pytest.mark.parametrize("d", DIMS)
def test_bound_and_layout(d):
    rng = np.random.default_rng(d)
    P = (d + 15) // 16 * 16
    codes, first = _rows(rng, d, P, 200)
    n = codes.shape[0]
    nib, bit, R, rho = _plane(codes, d)
    c64 = codes.astype(np.int64)
    # per-row caches as the index holds them (values of the sizes real rows have; the bound must hold for any non-negative ones)
    s_r = (rng.random(n) * 0.05 + 1e-3).astype(F)
    s_r[-1] = F(0)                                   # the zero row
    T_r = np.array([_up(float(s_r[i]) * np.sqrt(float((c64[i] ** 2).sum()))) for i in range(n)], F)
    E_r = (s_r * F(0.3 * np.sqrt(d))).astype(F)
    invn = (1.0 / np.maximum(s_r.astype(np.float64) * np.sqrt((c64 ** 2).sum(axis=1)), 1e-3)).astype(F)
    absmin = F(2.0 ** -100 * (d + 8))
    worst = 0.0
    for qc in _queries(rng, d, codes, rho, first):
        C = c64[:, :d] @ qc
        S = _sum_cq_u(nib, bit, qc)
        C5 = 8 * S - 124 * int(qc.sum())
        assert np.array_equal(C - C5, rho @ qc), "the decode of the packed planes is not sum c_q (8u - 124)"
        q_cn = _up(np.sqrt(float((qc ** 2).sum())))
        Uf = (q_cn * R).astype(F)
        U = Uf.astype(np.float64)
        assert (C5 - U <= C).all() and (C <= C5 + U).all()
        if (qc != 0).any():
            worst = max(worst, float(np.max(np.abs(C - C5) / np.maximum(U, 1e-30))))
        s_q = F(0.02)
        k = (s_q * s_r).astype(F)
        N_q = _up(float(s_q) * np.sqrt(float((qc ** 2).sum())) * 1.001)
        D_q = _up(float(s_q) * 0.29 * np.sqrt(d))
        c0 = (((N_q * E_r).astype(F) + (D_q * T_r).astype(F)).astype(F) * F(1 + 2.0 ** -10)).astype(F)
        for cosine in (False, True):
            q_inv = F(1.0 / max(float(N_q), 1e-6)) if cosine else F(1)
            for bias in (None, (rng.random(n) * 0.05).astype(F), (-rng.random(n) * 5).astype(F)):
                hi = _hi_int8(C, k, c0, absmin, cosine, invn, q_inv, bias)
                hi5, ch, cl = _hi5(C5, Uf, k, c0, absmin, cosine, invn, q_inv, bias)
                assert (ch.astype(np.float64) >= C).all() and (cl.astype(np.float64) <= C).all()
                assert np.isfinite(hi5).all() and (hi5 >= hi).all(), f"d={d} cosine={cosine}: hi5 < hi"
    assert worst > 0.99, f"the adversarial rows should make the residual bound tight, reached {worst}"
