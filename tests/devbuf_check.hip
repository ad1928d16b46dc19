// devbuf_check.hip -- host program of tests/test_devbuf.py: DevBuf (csrc/hdb_devbuf.h) over a counting allocator.  No GPU call is made.
// The fake Mem hands out malloc'ed blocks, counts live blocks and bytes, numbers every synchronise and free, and can be told to fail
// the k-th allocation or the next copy.  Swept: old capacity x new capacity x keep x fault, for alloc, grow_keep and the "two locals,
// then swap" pattern of buffers that change together.  Checked after success: the kept prefix, the exact capacity, one live block
// per buffer, a synchronise before the old block went; after a failed grow_keep: pointer, capacity and contents unchanged; after a
// failed alloc: empty; at every scope exit and at program exit: no live block (the fake's own count is the leak check).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <map>

#include "hdb_devbuf.h"
#include "plan_check.h"

static long g_points = 0;

struct FakeMem {
    static std::map<void*, size_t> live;      // block -> bytes
    static size_t live_bytes;
    static long allocs, frees, copies, syncs; // calls so far
    static long clock, last_sync;             // every sync and free takes a tick; last_sync: the tick of the latest sync
    static long fail_alloc, fail_copy;        // fail the k-th allocation from now (1 = the next), the next copy (1); 0 = none
    static hipError_t alloc(void** p, size_t bytes) {
        ++allocs;
        if (fail_alloc > 0 && --fail_alloc == 0) { *p = nullptr; return hipErrorOutOfMemory; }
        *p = std::malloc(bytes ? bytes : 1);
        live[*p] = bytes; live_bytes += bytes;
        return hipSuccess;
    }
    static hipError_t free(void* p) {
        ++frees; ++clock;
        auto it = live.find(p);
        if (it == live.end()) { CHECK(false, "free of a block that is not live"); return hipErrorInvalidValue; }
        live_bytes -= it->second; live.erase(it);
        std::free(p);
        return hipSuccess;
    }
    static hipError_t copy(void* dst, const void* src, size_t bytes, hipStream_t) {
        ++copies;
        if (fail_copy > 0 && --fail_copy == 0) return hipErrorInvalidValue;
        CHECK(live.count(dst) && live[dst] >= bytes, "copy past the new block");
        auto s = live.find(const_cast<void*>(src));
        CHECK(s != live.end() && s->second >= bytes, "copy past the old block");
        std::memcpy(dst, src, bytes);
        return hipSuccess;
    }
    static hipError_t sync() { ++syncs; last_sync = ++clock; return hipSuccess; }
    static void arm(long k_alloc, long copy) { fail_alloc = k_alloc; fail_copy = copy; }
};
std::map<void*, size_t> FakeMem::live;
size_t FakeMem::live_bytes = 0;
long FakeMem::allocs = 0, FakeMem::frees = 0, FakeMem::copies = 0, FakeMem::syncs = 0, FakeMem::clock = 0, FakeMem::last_sync = 0;
long FakeMem::fail_alloc = 0, FakeMem::fail_copy = 0;

typedef DevBuf<uint32_t, FakeMem> Buf;
static uint32_t pattern(size_t i, uint32_t salt) { return (uint32_t)(i * 2654435761u) ^ salt; }
static void fill(Buf& b, uint32_t salt) { for (size_t i = 0; i < b.cap; ++i) b.p[i] = pattern(i, salt); }
static bool holds(const uint32_t* p, size_t n, uint32_t salt) { for (size_t i = 0; i < n; ++i) if (p[i] != pattern(i, salt)) return false; return true; }

enum Fault { NONE, ALLOC1, ALLOC2, COPY, NFAULT };
static const char* const FAULT_NAME[] = {"none", "1st allocation", "2nd allocation", "copy"};
static void arm(int fault) { FakeMem::arm(fault == ALLOC1 ? 1 : fault == ALLOC2 ? 2 : 0, fault == COPY ? 1 : 0); }

// a buffer of `cap_old` elements holding pattern(salt); its setup is not part of the counted calls
static void make(Buf& b, size_t cap_old, uint32_t salt) {
    FakeMem::arm(0, 0);
    if (cap_old) { CHECK(b.alloc(cap_old) == hipSuccess, "setup"); fill(b, salt); }
}

static void check_alloc(size_t cap_old, size_t cap_new, int fault) {
    const size_t live0 = FakeMem::live.size();
    {
        Buf b; make(b, cap_old, 1u);
        uint32_t* const p0 = b.p;
        const long a0 = FakeMem::allocs, f0 = FakeMem::frees, s0 = FakeMem::syncs;
        arm(fault);
        const hipError_t e = b.alloc(cap_new);
        const bool failed = e != hipSuccess;
        if (cap_new <= cap_old) {
            CHECK(!failed && b.p == p0 && b.cap == cap_old, "alloc %zu -> %zu moved the buffer", cap_old, cap_new);
            CHECK(FakeMem::allocs == a0 && FakeMem::frees == f0 && FakeMem::syncs == s0, "alloc %zu -> %zu touched the allocator", cap_old, cap_new);
        } else if (fault == ALLOC1) {
            CHECK(failed && b.p == nullptr && b.cap == 0, "failed alloc %zu -> %zu left the buffer non-empty", cap_old, cap_new);
            CHECK(FakeMem::live.size() == live0, "failed alloc %zu -> %zu: %zu live blocks", cap_old, cap_new, FakeMem::live.size() - live0);
        } else {
            CHECK(!failed && b.p && b.cap == cap_new, "alloc %zu -> %zu: capacity %zu", cap_old, cap_new, b.cap);
            CHECK(FakeMem::live.size() == live0 + 1 && FakeMem::live[b.p] == cap_new * sizeof(uint32_t), "alloc %zu -> %zu: blocks or bytes", cap_old, cap_new);
            if (cap_old) CHECK(FakeMem::frees == f0 + 1 && FakeMem::syncs > s0, "alloc %zu -> %zu: the old block went without a synchronise", cap_old, cap_new);
            fill(b, 2u);          // every element is writable (AddressSanitizer watches the block's end)
        }
    }
    CHECK(FakeMem::live.size() == live0, "alloc %zu -> %zu (%s): a block outlived its buffer", cap_old, cap_new, FAULT_NAME[fault]);
}

static void check_grow_keep(size_t cap_old, size_t cap_new, size_t keep, int fault) {
    const size_t live0 = FakeMem::live.size();
    {
        Buf b; make(b, cap_old, 3u);
        uint32_t* const p0 = b.p;
        const long a0 = FakeMem::allocs, f0 = FakeMem::frees, s0 = FakeMem::syncs, c0 = FakeMem::copies;
        arm(fault);
        const hipError_t e = b.grow_keep(cap_new, keep, nullptr);
        const bool failed = e != hipSuccess;
        const bool copies = keep > 0 && cap_old > 0;
        if (cap_new <= cap_old) {
            CHECK(!failed && b.p == p0 && b.cap == cap_old && holds(b.p, cap_old, 3u), "grow_keep %zu -> %zu moved the buffer", cap_old, cap_new);
            CHECK(FakeMem::allocs == a0 && FakeMem::frees == f0 && FakeMem::syncs == s0 && FakeMem::copies == c0, "grow_keep %zu -> %zu touched the allocator", cap_old, cap_new);
        } else if (fault == ALLOC1 || (fault == COPY && copies)) {
            CHECK(failed, "grow_keep %zu -> %zu keep %zu (%s) reported success", cap_old, cap_new, keep, FAULT_NAME[fault]);
            CHECK(b.p == p0 && b.cap == cap_old && holds(b.p, cap_old, 3u), "failed grow_keep %zu -> %zu keep %zu (%s) changed the buffer", cap_old, cap_new, keep, FAULT_NAME[fault]);
            CHECK(FakeMem::live.size() == live0 + (cap_old ? 1 : 0), "failed grow_keep %zu -> %zu (%s) leaked", cap_old, cap_new, FAULT_NAME[fault]);
        } else {
            CHECK(!failed && b.p && b.cap == cap_new, "grow_keep %zu -> %zu: capacity %zu", cap_old, cap_new, b.cap);
            CHECK(FakeMem::live.size() == live0 + 1 && FakeMem::live[b.p] == cap_new * sizeof(uint32_t), "grow_keep %zu -> %zu: blocks or bytes", cap_old, cap_new);
            CHECK(holds(b.p, cap_old ? keep : 0, 3u), "grow_keep %zu -> %zu lost the first %zu elements", cap_old, cap_new, keep);
            CHECK(FakeMem::syncs > s0 && FakeMem::frees == f0 + (cap_old ? 1 : 0), "grow_keep %zu -> %zu: synchronise / free counts", cap_old, cap_new);
            fill(b, 4u);
        }
    }
    CHECK(FakeMem::live.size() == live0, "grow_keep %zu -> %zu keep %zu (%s): a block outlived its buffer", cap_old, cap_new, keep, FAULT_NAME[fault]);
}

// Two buffers that change together (the per-row caches, the shadow's codes and caches): new blocks in two locals, the kept rows
// copied by the caller, both swapped into the owner after the last step that can fail.  Any failure: the owner is as it was.
struct Pair { Buf a, b; };
static hipError_t grow_pair(Pair& own, size_t cap_new, size_t keep) {
    Buf a2, b2;
    hipError_t e = a2.alloc(cap_new);
    if (e == hipSuccess) e = b2.alloc(cap_new);
    if (e == hipSuccess && keep > 0 && own.a) e = FakeMem::copy(a2, own.a, keep * sizeof(uint32_t), nullptr);
    if (e == hipSuccess && keep > 0 && own.b) e = FakeMem::copy(b2, own.b, keep * sizeof(uint32_t), nullptr);
    if (e != hipSuccess) return e;                        // a2 / b2 free the new blocks
    own.a.swap(a2); own.b.swap(b2);
    return hipSuccess;                                    // a2 / b2 synchronise and free the old ones
}
static void check_pair(size_t cap_old, size_t cap_new, size_t keep, int fault) {
    const size_t live0 = FakeMem::live.size();
    {
        Pair own; make(own.a, cap_old, 5u); make(own.b, cap_old, 6u);
        uint32_t* const pa = own.a.p; uint32_t* const pb = own.b.p;
        const long f0 = FakeMem::frees, s0 = FakeMem::syncs;
        const size_t held = cap_old ? 2 : 0;
        arm(fault);
        const hipError_t e = grow_pair(own, cap_new, keep);
        const bool copies = keep > 0 && cap_old > 0;
        if (fault == ALLOC1 || fault == ALLOC2 || (fault == COPY && copies)) {
            CHECK(e != hipSuccess, "pair %zu -> %zu (%s) reported success", cap_old, cap_new, FAULT_NAME[fault]);
            CHECK(own.a.p == pa && own.b.p == pb && own.a.cap == cap_old && own.b.cap == cap_old, "failed pair %zu -> %zu (%s) changed the owner", cap_old, cap_new, FAULT_NAME[fault]);
            CHECK(holds(own.a.p, cap_old, 5u) && holds(own.b.p, cap_old, 6u), "failed pair %zu -> %zu (%s) changed the contents", cap_old, cap_new, FAULT_NAME[fault]);
            CHECK(FakeMem::live.size() == live0 + held, "failed pair %zu -> %zu (%s) leaked", cap_old, cap_new, FAULT_NAME[fault]);
        } else {
            CHECK(e == hipSuccess && own.a.cap == cap_new && own.b.cap == cap_new, "pair %zu -> %zu: capacities", cap_old, cap_new);
            CHECK(FakeMem::live.size() == live0 + 2, "pair %zu -> %zu: %zu live blocks", cap_old, cap_new, FakeMem::live.size() - live0);
            const size_t kept = cap_old ? (keep < cap_new ? keep : cap_new) : 0;
            CHECK(holds(own.a.p, kept, 5u) && holds(own.b.p, kept, 6u), "pair %zu -> %zu lost the first %zu elements", cap_old, cap_new, keep);
            CHECK(FakeMem::frees == f0 + (long)held && FakeMem::syncs >= s0 + (long)held, "pair %zu -> %zu: an old block went without a synchronise", cap_old, cap_new);
            fill(own.a, 7u); fill(own.b, 8u);
        }
    }
    CHECK(FakeMem::live.size() == live0, "pair %zu -> %zu keep %zu (%s): a block outlived its buffer", cap_old, cap_new, keep, FAULT_NAME[fault]);
}

// reset, swap and the order of synchronise and free: no held block is freed without a synchronise after the last call that used it
static void check_small() {
    {
        Buf a, b; make(a, 64, 9u);
        CHECK(!b && b.cap == 0, "a fresh buffer is not empty");
        a.swap(b);
        CHECK(!a && a.cap == 0 && b.cap == 64 && holds(b, 64, 9u), "swap");
        const long s0 = FakeMem::syncs, f0 = FakeMem::frees;
        a.reset();
        CHECK(FakeMem::syncs == s0 && FakeMem::frees == f0, "reset of an empty buffer touched the allocator");
        const long t0 = FakeMem::clock;
        b.reset();
        CHECK(!b && b.cap == 0 && FakeMem::frees == f0 + 1 && FakeMem::last_sync == t0 + 1 && FakeMem::clock == t0 + 2, "reset: synchronise, then free");
    }
    {   // grow_keep: the synchronise lies between the copy and the free of the old block
        Buf a; make(a, 3, 10u);
        const long t0 = FakeMem::clock;
        CHECK(a.grow_keep(1000, 3, nullptr) == hipSuccess && FakeMem::last_sync == t0 + 1 && FakeMem::clock == t0 + 2, "grow_keep: synchronise, then free");
    }
}

int main() {
    const size_t olds[] = {0, 1, 3, 64, 1000}, news[] = {1, 3, 64, 1000, 1500};
    for (size_t cap_old : olds)
        for (size_t cap_new : news)
            for (int fault = NONE; fault < NFAULT; ++fault) {
                check_alloc(cap_old, cap_new, fault);
                const size_t keeps[] = {0, 1, cap_old};
                for (size_t keep : keeps) {
                    if (keep > cap_old) continue;         // (keep = 1 of an empty buffer)
                    check_grow_keep(cap_old, cap_new, keep, fault);
                    if (cap_new >= cap_old) check_pair(cap_old, cap_new, keep, fault);      // (the pattern always takes new blocks: only growth keeps rows)
                    g_points += 3;
                }
            }
    check_small();
    FakeMem::arm(0, 0);
    CHECK(FakeMem::live.empty() && FakeMem::live_bytes == 0, "at exit: %zu live blocks, %zu bytes", FakeMem::live.size(), FakeMem::live_bytes);
    std::printf("devbuf_check: %ld points, %ld allocations, %ld frees\n", g_points, FakeMem::allocs, FakeMem::frees);
    return check_done();
}
