// plane_queue_check.hip -- the pending queue between the two stages of the plane pass (hdb_plane_vt_map and its parts,
// HdbPlanePending, csrc/hdb_caps.h) on the host: a stand-alone program, no GPU call.
//
// Stage A of hdb_quant_plane_scan_kernel (csrc/hdb_quant.hip) appends the rows its four-bit bound keeps to a wave-private queue of
// HQ_PL_QUEUE = 48 entries; while 16 or more are pending, stage B takes the top 16 as one virtual tile of bit words -- lane l takes
// words l + 64 j, j < J = ceil(U / 4), word f of pending row f / U, unit f % U, at pl_bit[row U + unit] -- and what is left after
// the walk goes as one ragged tile.  The rows stage B keeps go to the survivor queue (48 entries too), drained 16 at a time.
// The program checks that
//   for U = 1 .. 16 and every f a lane can hold (f < 64 J): hdb_plane_vt_map gives slot f / U and query offset 2 (f % U) for
//     f < 16 U and slot 16 (no row) past it, and hdb_plane_vt_word is row U + f % U against plain division, for row numbers up to
//     2^32 - 1 (the word index then passes 2^31);
//   a model of the two queues, run over random steps (0 .. 32 kept rows a step, stage B keeping each with a probability that
//     varies by sequence), steps that keep all 32, steps that keep none and alternations of them: the pending queue never holds more
//     than 48 entries nor 16 or more after a step, the survivor queue never more than 48 nor 16 or more after a flush, every
//     entry is flushed exactly once -- the ragged end included -- and every survivor is drained exactly once;
//   an entry is 32 bytes with the row first (the flush's address loads read entry.row alone).
// It prints "maps M", "steps S", "entries E", "survivors V" and " F failures"; exit status 1 on any failure.
#include "hdb_common.h"
#include "plan_check.h"
#include <cstddef>
#include <cstdio>
#include <vector>

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { g_state = g_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(g_state >> 33); }

static const int QUEUE = 48;                 // HQ_PL_QUEUE (hdb_quant.hip), both queues

struct Model {
    std::vector<int> pend, surv;             // entry ids; the kernel takes both from the top
    std::vector<int> flushed, drained, kept; // per entry id
    long max_pend = 0, max_surv = 0;
    uint32_t keep_of_256;                    // stage B keeps an entry with probability keep_of_256 / 256
    void drain(int m) {
        CHECK(m >= 1 && m <= 16 && (int)surv.size() >= m, "a drain of %d from %zu", m, surv.size());
        for (int i = 0; i < m; ++i) { ++drained[(size_t)surv.back()]; surv.pop_back(); }
    }
    void flush(int m) {                      // the top m pending entries as one virtual tile
        CHECK(m >= 1 && m <= 16 && (int)pend.size() >= m, "a flush of %d from %zu", m, pend.size());
        CHECK(surv.size() < 16, "%zu survivors wait at a flush", surv.size());
        const size_t base = pend.size() - (size_t)m;
        for (int s = 0; s < m; ++s) {
            const int id = pend[base + (size_t)s];
            ++flushed[(size_t)id];
            if ((rnd() & 255u) < keep_of_256) { kept[(size_t)id] = 1; surv.push_back(id); }
        }
        pend.resize(base);
        if ((long)surv.size() > max_surv) max_surv = (long)surv.size();
        CHECK((int)surv.size() <= QUEUE, "%zu survivors queued", surv.size());
        if (surv.size() >= 16) drain(16);
        CHECK(surv.size() < 16, "%zu survivors left by a flush", surv.size());
    }
    void step(int k) {                       // a step of the stream whose four-bit bound keeps k of its 32 rows
        CHECK(pend.size() < 16, "%zu pending at a step", pend.size());
        for (int i = 0; i < k; ++i) {
            pend.push_back((int)flushed.size());
            flushed.push_back(0); drained.push_back(0); kept.push_back(0);
        }
        if ((long)pend.size() > max_pend) max_pend = (long)pend.size();
        CHECK((int)pend.size() <= QUEUE, "%zu pending", pend.size());
        while (pend.size() >= 16) flush(16);
    }
    void end() {                             // the end of the walk: a ragged tile, then what the survivor queue still holds
        if (!pend.empty()) flush((int)pend.size());
        if (!surv.empty()) drain((int)surv.size());
    }
};

int main() {
    long maps = 0;
    const int64_t rows[6] = {0, 1, 8208, 70000, 0x7FFFFFFFll, 0xFFFFFFFFll};
    for (uint32_t U = 1; U <= 16; ++U) {
        const uint32_t J = (U + 3u) / 4u;
        for (uint32_t f = 0; f < 64u * J; ++f) {
            const uint32_t m = hdb_plane_vt_map(f, U);
            if (f < 16u * U) {
                CHECK(hdb_plane_vt_slot(m) == f / U && hdb_plane_vt_qoff(m) == 2u * (f % U), "U %u f %u: slot %u offset %u", U, f,
                      hdb_plane_vt_slot(m), hdb_plane_vt_qoff(m));
                CHECK(hdb_plane_vt_slot(m) < 16u && hdb_plane_vt_qoff(m) + 1u < 2u * U, "U %u f %u: beyond the tile or the query words", U, f);
                for (int64_t row : rows)
                    CHECK(hdb_plane_vt_word(row, m, U) == row * (int64_t)U + (int64_t)(f % U), "U %u f %u row %lld: word %lld", U, f, (long long)row,
                          (long long)hdb_plane_vt_word(row, m, U));
            } else {
                CHECK(hdb_plane_vt_slot(m) == 16u && hdb_plane_vt_qoff(m) == 0u, "U %u f %u past the tile: slot %u offset %u", U, f, hdb_plane_vt_slot(m),
                      hdb_plane_vt_qoff(m));
            }
            ++maps;
        }
        // the 16 U words of a virtual tile are those of a nibble tile: every (slot, unit) exactly once
        std::vector<int> seen(16u * U, 0);
        for (uint32_t f = 0; f < 16u * U; ++f) {
            const uint32_t m = hdb_plane_vt_map(f, U);
            ++seen[hdb_plane_vt_slot(m) * U + (hdb_plane_vt_qoff(m) >> 1)];
        }
        for (uint32_t i = 0; i < 16u * U; ++i) CHECK(seen[i] == 1, "U %u: word %u taken %d times", U, i, seen[i]);
    }
    CHECK(sizeof(HdbPlanePending) == 32 && offsetof(HdbPlanePending, row) == 0 && offsetof(HdbPlanePending, t_s) == 16, "the entry's layout");

    long steps = 0, entries = 0, survivors = 0;
    for (int seq = 0; seq < 64; ++seq) {
        Model q;
        q.keep_of_256 = seq % 4 == 0 ? 256u : seq % 4 == 1 ? 0u : seq % 4 == 2 ? 32u : 200u;
        const int kind = seq / 4 % 4, nsteps = 200 + (int)(rnd() % 100u);
        for (int s = 0; s < nsteps; ++s) {
            int k;
            switch (kind) {
            case 0: k = (int)(rnd() % 33u); break;                                   // anything
            case 1: k = 32; break;                                                   // every row kept: two flushes a step
            case 2: k = (s % 7 == 3) ? 32 : 0; break;                                // nothing, then a full step
            default: k = (rnd() % 8u == 0u) ? (int)(rnd() % 33u) : (int)(rnd() % 5u); break;      // about one row in eight
            }
            if (seq >= 48 && s + 1 == nsteps) k = 1 + seq % 15;                      // (a ragged end for certain)
            q.step(k);
            ++steps;
        }
        q.end();
        CHECK(q.pend.empty() && q.surv.empty(), "seq %d: %zu pending, %zu survivors left", seq, q.pend.size(), q.surv.size());
        CHECK(q.max_pend <= QUEUE && q.max_surv <= QUEUE, "seq %d: %ld pending, %ld survivors at most", seq, q.max_pend, q.max_surv);
        if (kind == 1) CHECK(q.max_pend >= 32, "seq %d: full steps reach %ld entries", seq, q.max_pend);
        for (size_t id = 0; id < q.flushed.size(); ++id) {
            CHECK(q.flushed[id] == 1, "seq %d: entry %zu flushed %d times", seq, id, q.flushed[id]);
            CHECK(q.drained[id] == q.kept[id], "seq %d: entry %zu kept %d drained %d", seq, id, q.kept[id], q.drained[id]);
            survivors += q.kept[id];
        }
        entries += (long)q.flushed.size();
    }
    // no step keeps a row: nothing is ever queued, flushed or drained
    {
        Model q; q.keep_of_256 = 256u;
        for (int s = 0; s < 100; ++s) { q.step(0); ++steps; }
        q.end();
        CHECK(q.flushed.empty() && q.max_pend == 0 && q.max_surv == 0, "an empty walk queued something");
    }
    std::printf("maps %ld\nsteps %ld\nentries %ld\nsurvivors %ld\n", maps, steps, entries, survivors);
    return check_done();
}
