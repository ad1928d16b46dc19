// group_plan_check.hip -- host program of tests/test_grouped_host.py: the schedule of hdb_topk_grouped_host (csrc/hdb_group_plan.h)
// and the workspace of its exact pass (TopkWs with the per-group maxima, csrc/hdb_ws.h) over a grid.  No GPU call is made.
//   rounds     over (n, k, oversample, fast rounds): at most two rounds, none when group_fast_rounds = 0, rows per query never above
//              min(n, HDB_MAX_K), strictly increasing, the first round = min(n, HDB_MAX_K, k * oversample clamped to 1 .. 64);
//   exact plan over (n, d, dtype, metric, nq, k, groups, mask): the plan of group_exact_call has the exact shape whatever the size of
//              the matrix (matrices of up to HDB_CAND_CAP rows included, on the VALU scan), its chunk keeps scores AND maxima inside
//              exact_bytes, and the same call without groups plans exactly as it did (no maxima, the small path where it was);
//   workspace  the size the dry run reports is where the placing run ends; the maxima and the flag word are 256-byte aligned, hold
//              their bytes, lie behind the score buffer and inside the reported size, and exist only for a grouped plan.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <sys/mman.h>

#include "hdb_group_plan.h"
#include "../include/hyperdb_hip.h"
#include "plan_check.h"

static long g_points = 0;

int main() {
    // ---- the round schedule ----
    const int64_t ns[] = {1, 2, 7, 100, 2047, 2048, 2049, 8192, 8193, 20001, 10000000};
    const int32_t ks[] = {1, 2, 10, 100, 512, 513, 2047, 2048};
    const int64_t oss[] = {-3, 0, 1, 2, 4, 7, 64, 65, 1000};
    const int64_t frs[] = {0, 1, 2, 3};
    for (int64_t n : ns) for (int32_t k : ks) for (int64_t os : oss) for (int64_t fr : frs) {
        ++g_points;
        const GroupRounds g = group_rounds(n, k, os, fr);
        const int64_t cap = std::min<int64_t>(n, HDB_MAX_K);
        CHECK(g.rounds >= 0 && g.rounds <= HDB_GROUP_ROUNDS_MAX, "n %ld k %d os %ld fr %ld: %d rounds", (long)n, k, (long)os, (long)fr, g.rounds);
        if (fr == 0) CHECK(g.rounds == 0, "n %ld k %d: %d rounds with group_fast_rounds = 0", (long)n, k, g.rounds);
        else CHECK(g.rounds >= 1 && g.rounds <= fr, "n %ld k %d fr %ld: %d rounds", (long)n, k, (long)fr, g.rounds);
        int32_t prev = 0;
        for (int r = 0; r < g.rounds; ++r) {
            CHECK(g.kr[r] >= 1 && (int64_t)g.kr[r] <= cap, "n %ld k %d os %ld: round %d takes %d rows, the limit is %ld", (long)n, k, (long)os, r, g.kr[r], (long)cap);
            CHECK(g.kr[r] > prev, "n %ld k %d os %ld: round %d takes %d rows after %d", (long)n, k, (long)os, r, g.kr[r], prev);
            prev = g.kr[r];
        }
        if (g.rounds >= 1) {
            const int64_t osc = std::max<int64_t>(1, std::min<int64_t>(os, 64));
            CHECK((int64_t)g.kr[0] == std::min<int64_t>(cap, (int64_t)k * osc), "n %ld k %d os %ld: first round %d", (long)n, k, (long)os, g.kr[0]);
        }
        if (g.rounds == 2) CHECK((int64_t)g.kr[1] == std::min<int64_t>(cap, 4 * (int64_t)g.kr[0]), "n %ld k %d: second round %d after %d", (long)n, k, g.kr[1], g.kr[0]);
        if (fr >= 2 && g.rounds == 1) CHECK((int64_t)g.kr[0] == cap, "n %ld k %d os %ld: one round of %d rows although more exist", (long)n, k, (long)os, g.kr[0]);
    }
    // ---- the exact plan and its workspace ----
    const size_t RESERVE = (size_t)64 << 30;     // address space only: never touched
    char* base = (char*)mmap(nullptr, RESERVE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) { std::printf("mmap failed\n"); return 2; }
    const int64_t pn[] = {1, 12, 3000, 8192, 8193, 20001, 2000000};
    const int pd[] = {32, 64, 96, 384, 1024};
    const int dts[] = {HDB_F16, HDB_F32, HDB_F64, HDB_BF16, HDB_F8E4M3, HDB_I8, HDB_B1};
    const int mets[] = {HDB_DOT, HDB_COSINE, HDB_EUCLIDEAN, HDB_MANHATTAN, HDB_PEARSON};
    const int nqs[] = {1, 5, 300};
    const int32_t pk[] = {1, 100, 2048};
    const int64_t eb[] = {(int64_t)1 << 20, (int64_t)1 << 30};
    for (int64_t n : pn) for (int d : pd) for (int dt : dts) for (int me : mets) for (int nq : nqs) for (int32_t k : pk)
    for (int gsel = 0; gsel < 3; ++gsel) for (int mask = 0; mask < 2; ++mask) for (int64_t ebytes : eb) {
        ++g_points;
        const int64_t n_groups = gsel == 0 ? 1 : gsel == 1 ? std::max<int64_t>(1, n / 5) : n;
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = dt; f.qmode = 0; f.has_mask = mask != 0; f.has_bias = mask != 0; f.cus = 256; f.subset_m = mask ? std::max<int64_t>(1, n / 64) : 0;
        hdb_options o; o.exact_bytes = ebytes;
        const TopkPlan p = plan_topk(f, o, group_exact_call(nq, k, me, n_groups), [] { return true; });
        CHECK(group_exact_shape(p), "n %ld d %d dtype %d metric %d nq %d k %d: path %d exact %d small %d subset %d n_best %ld", (long)n, d, dt, me, nq, k,
              (int)p.path, (int)p.exact, (int)p.small, (int)p.subset, (long)p.n_best);
        CHECK(p.n_best == n_groups && p.stats.path == 2, "n %ld: n_best %ld for %ld groups, path stat %ld", (long)n, (long)p.n_best, (long)n_groups, (long)p.stats.path);
        CHECK(n > HDB_CAND_CAP || (!p.mfma && !p.l1tile), "n %ld: a matrix of up to HDB_CAND_CAP rows left the VALU scan", (long)n);
        CHECK(p.cq_max >= 1 && p.cq_max <= std::min(nq, 256), "n %ld nq %d: chunk of %d queries", (long)n, nq, p.cq_max);
        CHECK(p.cq_max == 1 || (int64_t)p.cq_max * (p.ld_n * 4 + n_groups * 8) <= ebytes, "n %ld groups %ld: a chunk of %d queries exceeds exact_bytes %ld", (long)n,
              (long)n_groups, p.cq_max, (long)ebytes);
        // the same call without groups: no maxima, and a small matrix keeps its small path
        TopkFacts f0 = f;
        f0.subset_m = 0;                 // (a list call would be planned as a matrix of the listed rows)
        const TopkPlan p0 = plan_topk(f0, o, TopkCall{nq, k, me, true, true}, [] { return true; });
        CHECK(p0.n_best == 0 && p0.small == (n <= HDB_CAND_CAP), "n %ld: the ungrouped call plans n_best %ld small %d", (long)n, (long)p0.n_best, (int)p0.small);
        // the workspace: size == placement, and the two grouped regions
        for (int grouped = 0; grouped < 2; ++grouped) {
            const TopkPlan& pp = grouped ? p : p0;
            const size_t size = ws_bytes_for<TopkWs>(nq, d, pp.W, pp.cq_max, pp.ld_scores, pp.ld_ks, pp.sort_n, (size_t)0, pp.n_best);
            CHECK(size <= RESERVE, "%zu bytes exceed the reservation", size);
            if (size > RESERVE) continue;
            TopkWs w; Bump b(base, size);
            w.lay(b, nq, d, pp.W, pp.cq_max, pp.ld_scores, pp.ld_ks, pp.sort_n, (size_t)0, pp.n_best);
            CHECK(b.off == size && b.off <= b.cap, "n %ld nq %d grouped %d: the placing run ends at %zu, the dry run at %zu", (long)n, nq, grouped, b.off, size);
            if (!grouped) { CHECK(!w.best && !w.gbad, "an ungrouped layout placed the per-group maxima"); continue; }
            CHECK(w.best && w.gbad, "a grouped layout without its maxima");
            if (!w.best || !w.gbad) continue;
            const size_t best_off = (size_t)((char*)w.best - base), bad_off = (size_t)((char*)w.gbad - base), best_bytes = (size_t)pp.cq_max * (size_t)n_groups * 8;
            const size_t sbuf_end = (size_t)((char*)w.sbuf - base) + (size_t)pp.cq_max * (size_t)pp.ld_scores * 4;
            CHECK(best_off % 256 == 0 && bad_off % 256 == 0, "maxima at %zu, flag at %zu: not 256-byte aligned", best_off, bad_off);
            CHECK(best_off >= sbuf_end, "the maxima at %zu overlap the scores, which end at %zu", best_off, sbuf_end);
            CHECK(!w.kbuf || best_off >= (size_t)((char*)w.kbuf - base) + (size_t)pp.cq_max * (size_t)pp.ld_ks * 4, "the maxima overlap the partial sums");
            CHECK(bad_off >= best_off + best_bytes && bad_off + 4 <= size, "maxima %zu + %zu, flag at %zu, size %zu", best_off, best_bytes, bad_off, size);
        }
    }
    std::printf("%ld points checked\n", g_points);
    return check_done();
}
