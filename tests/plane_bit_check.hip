// plane_bit_check.hip -- the two stages of the plane pass (hdb_plane_rho4, hdb_plane_r4_up, hdb_plane_interval, hdb_plane_div_u,
// csrc/hdb_caps.h) on the host: a stand-alone program, no GPU call.
//
// Stage A of hdb_quant_plane_scan_kernel (csrc/hdb_quant.hip) bounds a row from its nibbles, c = 16 n - 120 + rho4, with the
// tile's R4* >= ||rho4_r||; stage B reads the bit words of the rows stage A keeps and forms 2 S4 + S1.  The program packs rows the way
// hdb_quant_plane_rows_kernel does (nibble byte b of word i = elements 8i + b | 8i + 4 + b << 4, bit of element 4g + b at 8b + g),
// decodes them with the masks of the two stages, and checks that
//   for every code c in -127 .. 127: n = u >> 1 and the bit u & 1 give 8 (2 n + b) - 124 + rho5 = 16 n - 120 + rho4 = c, rho4 in
//     [-8, 7], and hdb_plane_rho4 is that rho4;
//   for U = 1 .. 16 (d = 32 U and two ragged widths below it), random and extreme code rows (all +-127, rho4 all -8, rho4 all 7,
//     zero) against random and extreme query codes: the masked dot products give S4 and S1 with 2 S4 + S1 the five-bit sum S, so
//     8 (2 S4 + S1) - 124 sum c_q is the integer of the one-stage decode; C4 = 16 S4 - 120 sum c_q and, with R4 = hdb_plane_r4_up of
//     the row's own sum of rho4^2 and N_c = ||c_q|| rounded up, hdb_plane_interval gives ch4 >= fl(C) >= cl4 (and in integers
//     |C - C4| <= N_c R4);
//   R4* of a tile (the float32 maximum of hdb_plane_r4_up over its rows) is at or above every row's sqrt(sum rho4^2);
//   hdb_plane_div_u(idx, hdb_plane_rcp_u(U)) = idx / U for every idx < 32 U, U = 1 .. 16.
// It prints "codes C", "rows R", "tiles T", "divisions D" and " F failures"; exit status 1 on any failure.
#include "hdb_common.h"
#include "plan_check.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }
static int rnd_code() { return (int)(rnd() % 255u) - 127; }

static int dot4(uint32_t a, const int8_t* q) {             // v_dot4_i32_i8 of an unsigned-nibble word against four query codes
    int s = 0;
    for (int b = 0; b < 4; ++b) s += (int)(int8_t)((a >> (8 * b)) & 0xFFu) * (int)q[b];
    return s;
}

// one row of P = 32 U code bytes (zero past d) against one query: every identity and the interval
static void one_row(const std::vector<int8_t>& c, const std::vector<int8_t>& q, int U, int d, float* r4_out, double* r4_true) {
    long long C = 0, qs = 0, qq = 0, S4 = 0, S1 = 0, S = 0, ss4 = 0;
    for (int un = 0; un < U; ++un) {
        uint32_t nw[4] = {0u, 0u, 0u, 0u}, bw = 0u;
        for (int w = 0; w < 8; ++w)
            for (int b = 0; b < 4; ++b) {
                const int e = 32 * un + 4 * w + b, cc = c[(size_t)e];
                const uint32_t u5 = (uint32_t)((cc >> 3) + 16);
                nw[w >> 1] |= (u5 >> 1) << (8 * b + 4 * (w & 1));
                bw |= (u5 & 1u) << (8 * b + w);
                S += (long long)u5 * q[(size_t)e];
                C += (long long)cc * q[(size_t)e];
                if (e < d) { const int r4 = hdb_plane_rho4(cc); ss4 += r4 * r4; }
            }
        const int8_t* qu = q.data() + 32 * un;
        for (int i = 0; i < 4; ++i) {                        // stage A's decode: no bit merge
            S4 += dot4(nw[i] & 0x0F0F0F0Fu, qu + 8 * i);
            S4 += dot4((nw[i] >> 4) & 0x0F0F0F0Fu, qu + 8 * i + 4);
        }
        for (int g = 0; g < 8; ++g) S1 += dot4((bw >> g) & 0x01010101u, qu + 4 * g);      // stage B's
    }
    for (size_t e = 0; e < q.size(); ++e) { qs += q[e]; qq += (long long)q[e] * q[e]; }
    CHECK(2 * S4 + S1 == S, "U %d d %d: 2 S4 + S1 = %lld, the five-bit sum %lld", U, d, 2 * S4 + S1, S);
    const long long C5 = 8 * (2 * S4 + S1) - 124 * qs, C4 = 16 * S4 - 120 * qs;
    CHECK(C5 == 8 * S - 124 * qs, "U %d d %d: C5", U, d);
    CHECK(std::llabs(C4) < (1ll << 31) && std::llabs(C5) < (1ll << 31), "U %d d %d: int32", U, d);
    float ncf = (float)std::sqrt((double)qq);                // N_c rounded up, as the query prep leaves it
    while ((double)ncf * (double)ncf < (double)qq) ncf = std::nextafterf(ncf, INFINITY);
    const float R4 = hdb_plane_r4_up((uint32_t)ss4);
    CHECK((double)R4 * (double)R4 >= (double)ss4, "U %d d %d: R4 %a below sqrt(%lld)", U, d, (double)R4, ss4);
    CHECK((double)std::llabs(C - C4) <= (double)ncf * (double)R4, "U %d d %d: |C - C4| = %lld above N_c R4 = %g", U, d, std::llabs(C - C4), (double)ncf * R4);
    float ch4, cl4;
    hdb_plane_interval((float)(int)C4, ncf * R4, ch4, cl4);
    const float fC = (float)(int)C;
    CHECK(ch4 >= fC && fC >= cl4, "U %d d %d: ch4 %a fl(C) %a cl4 %a", U, d, (double)ch4, (double)fC, (double)cl4);
    *r4_out = R4; *r4_true = std::sqrt((double)ss4);
}

int main() {
    long codes = 0;
    for (int c = -127; c <= 127; ++c) {
        const int h = c >> 3, u = h + 16, rho5 = c - (8 * h + 4), n = u >> 1, b = u & 1, rho4 = c - (16 * n - 120);
        CHECK(u >= 0 && u <= 31 && rho5 >= -4 && rho5 <= 3, "code %d: u %d rho5 %d", c, u, rho5);
        CHECK(8 * (2 * n + b) - 124 + rho5 == c && 16 * n - 120 + rho4 == c, "code %d", c);
        CHECK(rho4 >= -8 && rho4 <= 7 && rho4 == 8 * b - 4 + rho5 && rho4 == hdb_plane_rho4(c), "code %d: rho4 %d", c, rho4);
        ++codes;
    }

    long rows = 0, tiles = 0;
    for (int U = 1; U <= 16; ++U) {
        const int P = 32 * U;
        const int ds[3] = {P, P - 7 > 0 ? P - 7 : 1, P - 16 > 0 ? P - 16 : P};
        for (int d : ds) {
            // query codes: random, all 127, all -127, alternating, one element
            std::vector<std::vector<int8_t>> qs;
            for (int kind = 0; kind < 6; ++kind) {
                std::vector<int8_t> q((size_t)P, 0);
                for (int e = 0; e < d; ++e)
                    q[(size_t)e] = (int8_t)(kind < 2 ? rnd_code() : kind == 2 ? 127 : kind == 3 ? -127 : kind == 4 ? ((e & 1) ? 127 : -127) : (e == d / 3 ? 127 : 0));
                qs.push_back(q);
            }
            // a tile of 16 code rows: random, all +-127, rho4 all -8 (c = 16 n - 128), rho4 all 7 (c = 16 n - 113), zero
            std::vector<std::vector<int8_t>> tile;
            for (int r = 0; r < 16; ++r) {
                std::vector<int8_t> c((size_t)P, 0);
                for (int e = 0; e < d; ++e) {
                    int v;
                    switch (r) {
                    case 0: v = 127; break;
                    case 1: v = -127; break;
                    case 2: v = (e & 1) ? 127 : -127; break;
                    case 3: v = 16 * (int)(1 + rnd() % 15u) - 128; break;            // rho4 = -8, c in -112 .. 112
                    case 4: v = 16 * (int)(rnd() % 16u) - 113; break;                // rho4 = 7, c in -113 .. 127
                    case 5: v = 0; break;
                    case 6: v = -8; break;                                           // rho4 = -8 beside the padding's own
                    default: v = rnd_code(); break;
                    }
                    c[(size_t)e] = (int8_t)v;
                }
                tile.push_back(c);
            }
            for (const auto& q : qs) {
                float r4s = 0.f;
                double worst = 0.0;
                for (const auto& c : tile) {
                    float r4; double t;
                    one_row(c, q, U, d, &r4, &t);
                    r4s = std::fmax(r4s, r4); worst = std::fmax(worst, t);
                    ++rows;
                }
                CHECK((double)r4s >= worst, "U %d d %d: R4* %a below a row's %a", U, d, (double)r4s, worst);
                ++tiles;
            }
        }
    }
    for (uint32_t ss4 = 0; ss4 <= 64u * 512u; ++ss4) {
        const float r = hdb_plane_r4_up(ss4);
        CHECK((double)r * (double)r >= (double)ss4 && r - r == 0.f, "ss4 %u: %a", ss4, (double)r);
    }

    long divisions = 0;
    for (uint32_t U = 1; U <= 16; ++U) {
        const uint32_t rcp = hdb_plane_rcp_u(U);
        for (uint32_t idx = 0; idx < 32u * U; ++idx) { CHECK(hdb_plane_div_u(idx, rcp) == idx / U, "%u / %u", idx, U); ++divisions; }
    }
    std::printf("codes %ld\nrows %ld\ntiles %ld\ndivisions %ld\n", codes, rows, tiles, divisions);
    return check_done();
}
