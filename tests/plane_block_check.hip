// plane_block_check.hip -- the hot block of the plane pass (hdb_plane_k_*, hdb_plane_rc_*, hdb_plane_block_off, csrc/hdb_caps.h) on
// the host: a stand-alone program, no GPU call.
//
// hdb_quant_plane_rows_kernel (csrc/hdb_quant.hip) writes, per 16-row tile and metric flavour, 64 bytes of row terms with these
// functions and hdb_quant_plane_scan_kernel reads them back: the scale of a row rounded UP to bfloat16 (the lower side derived from
// it), the residual norm as a byte rc = ceil(2 R), and three float32 words of the tile.  The program checks that
//   for every bfloat16 bit pattern of a finite non-negative value b, and the float32 numbers just above and just below it (and a
//     float64 a hair above and below), k_hi = decode(encode(k)) >= k >= k_lo(k_hi), k_hi is the smallest such bfloat16, and
//     k_lo = k_hi (1 - 2^-7) exactly from 2^-126 on;
//   hdb_plane_up gives the smallest float32 at or above its argument;
//   for every integer sum of squares ss <= 16 x 512, rc = encode(ss) <= 182 decodes to 0.5 rc >= sqrt(ss), and rc is the smallest;
//   for U = 1 .. 16 and tiles 0 .. 40 the blocks [off, off + 64) of the two flavours and the reserved 128 bytes tile the 256 bytes of
//     a tile of 16 records (16 bytes per row whatever U is) without overlap, inside hdb_plane_rec_bytes(rows) for a ragged row count.
// It prints "patterns P", "sums S", "tiles T" and " F failures"; exit status 1 on any failure.
#include "hdb_common.h"
#include "plan_check.h"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

static float bf(uint32_t code) { uint32_t u = code << 16; float f; std::memcpy(&f, &u, 4); return f; }

static void one_k(double k, uint32_t code_of_b) {
    const uint32_t c = hdb_plane_k_encode(k);
    const float k_hi = hdb_plane_k_hi(c), k_lo = hdb_plane_k_lo(k_hi);
    CHECK(c <= 0x7F80u, "k %a near %04x: code %04x", k, code_of_b, c);
    CHECK((double)k_hi >= k && k >= (double)k_lo, "k %a near %04x: k_hi %a k_lo %a", k, code_of_b, (double)k_hi, (double)k_lo);
    if (c > 0u) CHECK((double)bf(c - 1u) < k, "k %a near %04x: %04x is not the smallest", k, code_of_b, c);
    if (c < 0x7F80u && k_hi >= 0x1p-126f) CHECK((double)k_lo == (double)k_hi * (1.0 - 0x1p-7), "k %a: k_lo %a is not exact", k, (double)k_lo);
    if (k_hi < 0x1p-126f) CHECK(k_lo == 0.f, "k %a: k_lo %a below the normal range", k, (double)k_lo);
    if (k <= 3.0e38) {
        const float up = hdb_plane_up(k);
        CHECK((double)up >= k && (up == 0.f || (double)std::nextafterf(up, 0.f) < k), "up(%a) = %a", k, (double)up);
    }
}

int main() {
    long patterns = 0;
    for (uint32_t code = 0; code < 0x7F80u; ++code) {            // every finite non-negative bfloat16
        const float b = bf(code);
        one_k((double)b, code);
        CHECK(hdb_plane_k_encode((double)b) == code, "%04x does not encode to itself", code);
        const float above = std::nextafterf(b, INFINITY), below = std::nextafterf(b, -INFINITY);
        if (above - above == 0.f) one_k((double)above, code);
        if (below >= 0.f) one_k((double)below, code);
        one_k(std::nextafter((double)b, INFINITY), code);
        if (b > 0.f) one_k(std::nextafter((double)b, 0.0), code);
        ++patterns;
    }
    one_k(0x1p-160, 0); one_k(0.0, 0);
    CHECK(hdb_plane_k_encode(0x1p-160) == 1u && hdb_plane_k_encode(0.0) == 0u && hdb_plane_k_encode(1e300) == 0x7F80u, "edges");

    long sums = 0;
    uint32_t rc_max = 0;
    for (uint32_t ss = 0; ss <= 16u * 512u; ++ss) {
        const uint32_t rc = hdb_plane_rc_encode(ss);
        const double R = (double)hdb_plane_rc_decode(rc);
        CHECK(rc <= 182u && R == 0.5 * rc, "ss %u: rc %u", ss, rc);
        CHECK(R * R >= (double)ss, "ss %u: rc %u decodes below sqrt(ss)", ss, rc);            // (R^2 = rc^2 / 4 is exact)
        if (rc > 0u) CHECK((double)(rc - 1u) * (rc - 1u) < 4.0 * ss, "ss %u: rc %u is not the smallest", ss, rc);
        rc_max = rc > rc_max ? rc : rc_max;
        ++sums;
    }
    CHECK(rc_max == 182u, "largest code %u", rc_max);

    long tiles = 0;
    for (int U = 1; U <= 16; ++U) {
        const int64_t rows = 16 * 40 + U;                          // a ragged last tile: 41 tiles
        const int64_t bytes = hdb_plane_rec_bytes(rows);
        CHECK(bytes == 41 * 256 && bytes >= rows * 16, "U %d: %lld bytes", U, (long long)bytes);
        std::vector<unsigned char> used((size_t)bytes, 0);
        for (int64_t t = 0; t * 16 < rows; ++t) {
            for (int fl = 0; fl < 2; ++fl) {
                const int64_t off = hdb_plane_block_off(t, fl);
                CHECK(off >= t * 256 && off + HDB_PLANE_BLOCK_BYTES <= t * 256 + 128 && off % 64 == 0, "U %d tile %lld flavour %d", U, (long long)t, fl);
                for (int b = 0; b < HDB_PLANE_BLOCK_BYTES; ++b) {
                    if (off + b < 0 || off + b >= bytes) { CHECK(false, "U %d tile %lld: outside the array", U, (long long)t); break; }
                    CHECK(used[(size_t)(off + b)] == 0, "U %d tile %lld flavour %d: overlap", U, (long long)t, fl);
                    used[(size_t)(off + b)] = 1;
                }
            }
            for (int b = 128; b < HDB_PLANE_TILE_BYTES; ++b) { CHECK(used[(size_t)(t * 256 + b)] == 0, "reserved"); used[(size_t)(t * 256 + b)] = 1; }
            ++tiles;
        }
        long holes = 0;
        for (unsigned char u : used) holes += u ? 0 : 1;
        CHECK(holes == 0, "U %d: %ld bytes in no block", U, holes);
    }
    // the fields of a block lie inside it, one after the other
    CHECK(HDB_PLANE_BLOCK_K == 0 && HDB_PLANE_BLOCK_RC == 32 && HDB_PLANE_BLOCK_TILE == 48 && HDB_PLANE_BLOCK_TILE + 16 == HDB_PLANE_BLOCK_BYTES, "fields");
    std::printf("patterns %ld\nsums %ld\ntiles %ld\n", patterns, sums, tiles);
    return check_done();
}
