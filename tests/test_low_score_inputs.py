"""Conditions on the INPUTS of tests/test_low_score_contract.py, checked on the CPU (no GPU, no library): the low-score generator
(tests/lowscore.py) must leave a float32 dot product comfortably inside the 1e-5 band -- else the GPU test would ask more than the
number format gives -- and must put the bf16-parts arithmetic outside it in the top 50 -- else the GPU test could not tell the two
flavours apart.  Neither condition looks at the code under test.  The measured ratios: profiles/low_score_contract.txt."""
import numpy as np
import pytest

import lowscore

# (384, 16) is the first 16 queries of (384, 64) on the same matrix: the 64-query case covers both
WIDTHS = sorted({d: max(nq for dd, nq in lowscore.CASES if dd == d) for d, _ in lowscore.CASES}.items())


def test_the_cases_share_matrices_as_claimed():
    V16, Q16 = lowscore.case(384, 16)
    V64, Q64 = lowscore.case(384, 64)
    assert np.array_equal(V16, V64) and np.array_equal(Q16, Q64[:16])
    for d, nq in lowscore.CASES:
        V, Q = lowscore.case(d, nq)
        assert V.shape == (lowscore.N_ROWS, d) and Q.shape == (nq, d) and V.dtype == np.float32 and Q.dtype == np.float32
        vn, qn = np.linalg.norm(V.astype(np.float64), axis=1), np.linalg.norm(Q.astype(np.float64), axis=1)
        # |v| is a chi of r = 32 degrees of freedom around vnorm = 20: 20 +- 2.5, its extremes over 20 005 rows near 10 and 31
        assert 5.0 < vn.min() and vn.max() < 40.0 and abs(np.median(vn) - 20.0) < 1.0 and np.allclose(qn, 2.0, rtol=1e-6)
        assert np.abs(lowscore.exact_dot(d, nq)).max() < 1.0          # the band is 1e-5 for every row and query


@pytest.mark.parametrize("d,nq", WIDTHS)
def test_float32_references_stay_inside_half_the_band(d, nq):
    """(i) np.matmul, per-query np.dot and a left-to-right float32 sum: every row of every query within 0.5 of the band."""
    V, Q = lowscore.case(d, nq)
    exact = lowscore.exact_dot(d, nq)
    band = lowscore.band_of(exact)
    worst = {"matmul": float((np.abs(lowscore.f32_matmul(V, Q) - exact) / band).max()),
             "dot": float((np.abs(lowscore.f32_dot_per_query(V, Q) - exact) / band).max()),
             "sequential": max(float((np.abs(lowscore.f32_sequential(V, Q[qi]) - exact[:, qi]) / band[:, qi]).max()) for qi in range(nq))}
    print(f"d={d} nq={nq} worst float32 error in bands: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 0.5 for v in worst.values()), worst


@pytest.mark.parametrize("d,nq", WIDTHS)
def test_the_parts_arithmetic_leaves_the_band_in_the_top_50(d, nq):
    """(ii) the five-product model returns a row outside the band in at least half the queries (d = 1024: at least one)."""
    V, Q = lowscore.case(d, nq)
    exact = lowscore.exact_dot(d, nq)
    model = lowscore.parts_model(V, Q)
    ratio = np.abs(model - exact) / lowscore.band_of(exact)
    hit = lowscore.queries_with_a_row_outside(model, exact)
    print(f"d={d} nq={nq} parts model: {100.0 * float((ratio > 1.0).mean()):.2f} % of rows outside, worst {float(ratio.max()):.2f} bands, "
          f"top-{lowscore.TOP_K} holds such a row in {hit} of {nq} queries")
    assert hit >= (1 if d == 1024 else (nq + 1) // 2), hit
    if d == 384:                                                      # ... and so does the 16-query case on its own
        assert lowscore.queries_with_a_row_outside(model[:, :16], exact[:, :16]) >= 8
