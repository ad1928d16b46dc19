// range_plan_check.hip -- host program of tests/test_range_host.py: how hdb_range_host cuts a call (csrc/hdb_range_plan.h) over a grid of
// (n, nq, exact_bytes), both chunk caps.  No GPU call is made.
//   chunk   1 <= cq <= min(nq, cap); cq x ld_n x 4 <= exact_bytes wherever one query's scores fit; ld_n is n rounded up to 4;
//           the chunks cover nq;
//   tiles   ntiles x HDB_RANGE_TILE >= n > (ntiles - 1) x HDB_RANGE_TILE;
//   call    the score pass's call asks for the exact shape of the multi-vector pass.
#include <cstdio>

#include "hdb_range_plan.h"
#include "plan_check.h"

int main() {
    long points = 0;
    const int64_t ns[] = {1, 3, 4, 4095, 4096, 4097, 8195, 100000, 262143, 262144, 10000000, 0xFFFFFFFFll};
    const int32_t nqs[] = {1, 4, 5, 127, 128, 129, 256, 257, 1000};
    const int64_t ebs[] = {(int64_t)1 << 20, (int64_t)3 << 20, (int64_t)1 << 30, (int64_t)1 << 34};
    for (int64_t n : ns) for (int32_t nq : nqs) for (int64_t eb : ebs) for (int cap : {128, 256}) {
        ++points;
        const RangePlan r = range_plan(n, nq, cap, eb);
        CHECK(r.ld_n >= n && r.ld_n < n + 4 && r.ld_n % 4 == 0, "n %ld: ld_n %ld", (long)n, (long)r.ld_n);
        CHECK(r.cq >= 1 && r.cq <= std::min<int>(nq, cap), "n %ld nq %d: chunk of %d queries", (long)n, nq, r.cq);
        const bool one_fits = r.ld_n * 4 <= eb;
        CHECK(!one_fits || (int64_t)r.cq * r.ld_n * 4 <= eb, "n %ld nq %d eb %ld: a chunk of %d queries exceeds exact_bytes", (long)n, nq, (long)eb, r.cq);
        CHECK(one_fits || r.cq == 1, "n %ld eb %ld: one query does not fit, cq %d", (long)n, (long)eb, r.cq);
        // the largest chunk the budget allows, not a smaller one
        CHECK(r.cq == std::min<int>(nq, cap) || (int64_t)(r.cq + 1) * r.ld_n * 4 > eb, "n %ld nq %d eb %ld: cq %d leaves room", (long)n, nq, (long)eb, r.cq);
        CHECK(r.ntiles * HDB_RANGE_TILE >= n && n > (r.ntiles - 1) * HDB_RANGE_TILE, "n %ld: %ld tiles", (long)n, (long)r.ntiles);
        const int64_t chunks = range_chunks(r, nq);
        CHECK(chunks * r.cq >= nq && (chunks - 1) * r.cq < nq, "nq %d: %ld chunks of %d", nq, (long)chunks, r.cq);
    }
    const TopkCall c = range_call(7, HDB_COSINE);
    CHECK(c.nq == 7 && c.k == 1 && c.metric == HDB_COSINE && c.exact && c.maxsim && c.has_status && c.n_groups == 0, "the score pass's call");
    CHECK(hdb_range_result_bytes(3) == 60 && HDB_RANGE_TILE == 4096 && HDB_RANGE_LDS_SORT == 8192, "the exported constants");
    std::printf("%ld points checked\n", points);
    return check_done();
}
