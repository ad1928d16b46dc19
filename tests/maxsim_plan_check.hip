// maxsim_plan_check.hip -- host program of tests/test_maxsim_host.py: how hdb_maxsim_host cuts a call (csrc/hdb_maxsim_plan.h), the
// call its score pass plans with and its workspace (MaxsimWs, csrc/hdb_ws.h) over a grid.  No GPU call is made.
//   blocks / chunks  over (n, n_groups, set sizes, chunk cap, exact_bytes): walking the call the way the executor does, every vector
//                    is in exactly one chunk, no chunk crosses a block's end, chunks do cut across set boundaries where sets are
//                    shorter than a chunk, 1 <= cq <= min(cap, 256), 1 <= sb <= min(ns, 256), sbuf + acc stay inside exact_bytes
//                    whenever one vector and one set fit, and maxsim_chunks counts the walk's chunks;
//   score pass       over (n, d, dtype, metric, vectors, mask): the plan of maxsim_call has the exact shape whatever the size of the
//                    matrix, never a row list, no per-group maxima, euclidean never on the matrix cores, and the same call without
//                    the flag plans as it did;
//   workspace        the size the dry run reports is where the placing run ends; acc and the selection's buffers are 256-byte
//                    aligned, hold their bytes, lie behind the score buffer and do not overlap.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <sys/mman.h>

#include "hdb_maxsim_plan.h"
#include "../include/hyperdb_hip.h"
#include "plan_check.h"

static long g_points = 0;

int main() {
    // ---- blocks and chunks ----
    const int64_t ns_rows[] = {1, 12, 3000, 8192, 8193, 20001, 70001, 2000000, 10000000};
    const int caps[] = {128, 256};
    const int64_t eb[] = {(int64_t)1 << 20, (int64_t)3 << 20, (int64_t)1 << 26, (int64_t)1 << 30};
    const std::vector<std::vector<int32_t>> shapes = {
        {1}, {33}, {1, 4, 5, 9, 33}, {300}, {2, 2, 2, 2, 2, 2, 2, 2}, std::vector<int32_t>(300, 1), std::vector<int32_t>(700, 3), {1000, 1, 1000}};
    bool cut_seen = false;
    for (int64_t n : ns_rows) for (int gsel = 0; gsel < 4; ++gsel) for (int cap : caps) for (int64_t ebytes : eb) for (const auto& T : shapes) {
        ++g_points;
        const int64_t n_groups = gsel == 0 ? 1 : gsel == 1 ? std::max<int64_t>(1, n / 100) : gsel == 2 ? std::max<int64_t>(1, n / 4) : n;
        const int32_t ns = (int32_t)T.size();
        std::vector<int32_t> off(1, 0);
        for (int32_t t : T) off.push_back(off.back() + t);
        const int32_t nv = off.back();
        const MaxsimPlan m = maxsim_plan(n, n_groups, ns, cap, ebytes);
        CHECK(m.cq >= 1 && m.cq <= std::min(cap, 256), "n %ld groups %ld: cq %d under cap %d", (long)n, (long)n_groups, m.cq, cap);
        CHECK(m.sb >= 1 && m.sb <= std::min<int32_t>(ns, 256), "n %ld groups %ld ns %d: sb %d", (long)n, (long)n_groups, ns, m.sb);
        CHECK(m.ld_n >= n && m.ld_n % 4 == 0 && m.ld_g >= n_groups && m.ld_g % 4 == 0, "leading dimensions %ld %ld", (long)m.ld_n, (long)m.ld_g);
        const int64_t one = m.ld_n * 4 + m.ld_g * 4, used = (int64_t)m.cq * m.ld_n * 4 + (int64_t)m.sb * m.ld_g * 4;
        if (one <= ebytes) CHECK(used <= ebytes, "n %ld groups %ld ns %d eb %ld: sbuf + acc = %ld (cq %d, sb %d)", (long)n, (long)n_groups, ns, (long)ebytes, (long)used, m.cq, m.sb);
        else CHECK(m.cq == 1 && m.sb == 1, "n %ld groups %ld: nothing fits, yet cq %d sb %d", (long)n, (long)n_groups, m.cq, m.sb);
        // the executor's walk
        std::vector<int> seen((size_t)nv, 0);
        int64_t chunks = 0;
        for (int32_t s0 = 0; s0 < ns; s0 += m.sb) {
            const int32_t sbn = std::min<int32_t>(m.sb, ns - s0), v_end = off[s0 + sbn];
            int32_t s_cur = s0;
            for (int32_t v0 = off[s0]; v0 < v_end; v0 += m.cq) {
                const int32_t cq = std::min<int32_t>(m.cq, v_end - v0);
                ++chunks;
                while (off[s_cur + 1] <= v0) ++s_cur;
                CHECK(s_cur >= s0 && s_cur < s0 + sbn && off[s_cur] <= v0, "chunk at %d: set %d outside block %d + %d", v0, s_cur, s0, sbn);
                int32_t s_last = s_cur;
                while (off[s_last + 1] < v0 + cq) ++s_last;
                CHECK(s_last < s0 + sbn, "chunk %d + %d runs into set %d beyond block %d + %d", v0, cq, s_last, s0, sbn);
                if (s_last > s_cur) cut_seen = true;
                for (int32_t v = v0; v < v0 + cq; ++v) ++seen[(size_t)v];
            }
        }
        bool once = true;
        for (int c : seen) once = once && c == 1;
        CHECK(once, "n %ld ns %d: a vector is in no chunk or in two", (long)n, ns);
        CHECK(chunks == maxsim_chunks(m, off.data(), ns), "walk %ld chunks, maxsim_chunks %ld", (long)chunks, (long)maxsim_chunks(m, off.data(), ns));
    }
    CHECK(cut_seen, "no chunk of the grid cut across a set boundary");
    // the documented shape: 52 vectors in five sets on 70 001 rows at 1 MiB -> cq = 3, one block, 18 chunks
    {
        const int32_t off[] = {0, 1, 5, 10, 19, 52};
        const MaxsimPlan m = maxsim_plan(70001, 400, 5, 256, (int64_t)1 << 20);
        CHECK(m.cq == 3 && m.sb == 5 && maxsim_chunks(m, off, 5) == 18, "cq %d sb %d chunks %ld", m.cq, m.sb, (long)maxsim_chunks(m, off, 5));
    }
    // ---- the score pass's plan and the workspace ----
    const size_t RESERVE = (size_t)64 << 30;     // address space only: never touched
    char* base = (char*)mmap(nullptr, RESERVE, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (base == (char*)MAP_FAILED) { std::printf("mmap failed\n"); return 2; }
    const int64_t pn[] = {1, 12, 3000, 8192, 8193, 20001, 2000000};
    const int pd[] = {32, 64, 128, 384, 1024};
    const int dts[] = {HDB_F16, HDB_F32, HDB_F64, HDB_BF16, HDB_F8E4M3, HDB_I8, HDB_B1};
    const int mets[] = {HDB_DOT, HDB_COSINE, HDB_EUCLIDEAN, HDB_MANHATTAN, HDB_PEARSON};
    const int nvs[] = {1, 9, 52, 300};
    for (int64_t n : pn) for (int d : pd) for (int dt : dts) for (int me : mets) for (int nv : nvs) for (int mask = 0; mask < 2; ++mask)
    for (int64_t ebytes : {(int64_t)1 << 20, (int64_t)1 << 30}) {
        ++g_points;
        TopkFacts f{};
        f.n = n; f.d = d; f.dtype = dt; f.qmode = 0; f.has_mask = mask != 0; f.has_bias = mask != 0; f.cus = 256; f.subset_m = mask ? std::max<int64_t>(1, n / 64) : 0;
        hdb_options o; o.exact_bytes = ebytes;
        const TopkPlan p = plan_topk(f, o, maxsim_call(nv, 10, me), [] { return true; });
        CHECK(maxsim_shape(p), "n %ld d %d dtype %d metric %d nv %d: path %d exact %d small %d subset %d n_best %ld", (long)n, d, dt, me, nv, (int)p.path,
              (int)p.exact, (int)p.small, (int)p.subset, (long)p.n_best);
        CHECK(p.stats.path == 2 && p.ld_n >= n, "n %ld: path stat %ld ld_n %ld", (long)n, (long)p.stats.path, (long)p.ld_n);
        CHECK(n > HDB_CAND_CAP || (!p.mfma && !p.l1tile), "n %ld: a matrix of up to HDB_CAND_CAP rows left the VALU scan", (long)n);
        // euclidean never takes the matrix cores here (their expansion cancels on near-duplicates and nothing re-scores them)
        CHECK(me != HDB_EUCLIDEAN || (!p.mfma && !p.ksplit && !p.f16_queries && !p.mask_fold), "n %ld d %d dtype %d nv %d: euclidean on the matrix cores", (long)n, d, dt, nv);
        // the same call without the flag plans as before: a small matrix keeps its small path
        TopkFacts f0 = f; f0.subset_m = 0;
        const TopkPlan p0 = plan_topk(f0, o, TopkCall{nv, 10, me, true, true}, [] { return true; });
        CHECK(p0.small == (n <= HDB_CAND_CAP) && p0.n_best == 0, "n %ld: the plain exact call plans small %d", (long)n, (int)p0.small);
        // the workspace
        const int64_t n_groups = std::max<int64_t>(1, n / 5);
        const int ns = std::min(nv, 5);
        const MaxsimPlan m = maxsim_plan(n, n_groups, ns, p.ksplit ? 128 : 256, ebytes);
        const int cq = std::min(m.cq, nv);
        const size_t size = ws_bytes_for<MaxsimWs>(nv, d, p.W, cq, p.ld_scores, p.ld_ks, m.sb, m.ld_g, ns);
        CHECK(size <= RESERVE, "%zu bytes exceed the reservation", size);
        if (size > RESERVE) continue;
        MaxsimWs w; Bump b(base, size);
        w.lay(b, nv, d, p.W, cq, p.ld_scores, p.ld_ks, m.sb, m.ld_g, ns);
        CHECK(b.off == size && b.off <= b.cap, "n %ld nv %d: the placing run ends at %zu, the dry run at %zu", (long)n, nv, b.off, size);
        const size_t sbuf_end = (size_t)((char*)w.t.sbuf - base) + (size_t)cq * (size_t)p.ld_scores * 4;
        const size_t acc_off = (size_t)((char*)w.acc - base), acc_end = acc_off + (size_t)m.sb * (size_t)m.ld_g * 4;
        const size_t voff_off = (size_t)((char*)w.voff - base), snan_off = (size_t)((char*)w.snan - base), cnt_off = (size_t)((char*)w.cnt - base);
        const size_t hist_off = (size_t)((char*)w.hist - base), tie_off = (size_t)((char*)w.tie_info - base), cand_off = (size_t)((char*)w.cand - base);
        CHECK(!w.t.best && !w.t.gbad && !w.t.sc1, "the multi-vector layout placed the grouped pass's maxima or the full sort's buffers");
        CHECK(acc_off % 256 == 0 && voff_off % 256 == 0 && snan_off % 256 == 0 && cnt_off % 256 == 0 && hist_off % 256 == 0 && cand_off % 256 == 0, "a region is not 256-byte aligned");
        CHECK(acc_off >= sbuf_end && (!w.t.kbuf || acc_off >= (size_t)((char*)w.t.kbuf - base) + (size_t)cq * (size_t)p.ld_ks * 4), "acc at %zu overlaps the scores", acc_off);
        CHECK(voff_off >= acc_end && snan_off >= voff_off + ((size_t)ns + 1) * 4 && cnt_off >= snan_off + (size_t)ns * 4, "acc / offsets / NaN words overlap");
        CHECK(hist_off >= cnt_off + (size_t)m.sb * HDB_CNT_STRIDE * 4 && tie_off >= hist_off + (size_t)m.sb * 4 * HDB_RADIX_BINS * 4 && cand_off >= tie_off + (size_t)m.sb * 16 &&
              cand_off + (size_t)m.sb * HDB_CAND_CAP * 8 <= size, "the selection's buffers overlap or leave the workspace");
    }
    std::printf("%ld points checked\n", g_points);
    return check_done();
}
