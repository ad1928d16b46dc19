// hdb_devbuf.h -- DevBuf, the one owner of a device allocation, and the two ways one grows.
//
// Every device block of the library (hdb_index, the group's query copies) is held by a DevBuf: allocated, grown and freed here and
// nowhere else.  The header knows the HIP runtime API's types and nothing of the library, so a host program can include it;
// tests/devbuf_check.hip runs the type over a counting allocator (the Mem policy) with injected failures.
//   alloc(cap_new)                keep-nothing growth: drops what it holds FIRST (lowest peak memory); failure leaves the buffer EMPTY
//   grow_keep(cap_new, keep, st)  new block, the first `keep` elements copied on `st`; failure leaves the buffer AS IT WAS
// Neither touches the allocator when cap_new <= cap.  Buffers that must change together are built in local DevBufs and swapped into
// their owner after the last step that can fail: an early return frees the new blocks, the owner keeps the old ones.
// One synchronisation rule: the device is synchronised before a held block is freed -- earlier launches may still read it (hipFree
// is documented to synchronise the device itself, so this orders nothing that was not ordered).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>

struct HipMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
    static hipError_t copy(void* dst, const void* src, size_t bytes, hipStream_t st) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st); }
    static hipError_t sync() { return hipDeviceSynchronize(); }
};

template <typename T, typename Mem = HipMem>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;                       // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { reset(); }
    operator T*() const { return p; }     // launch sites read `ix->inv_norm`
    void reset() {
        if (p) { (void)Mem::sync(); (void)Mem::free(p); }
        p = nullptr; cap = 0;
    }
    void swap(DevBuf& o) {
        T* const tp = p; p = o.p; o.p = tp;
        const size_t tc = cap; cap = o.cap; o.cap = tc;
    }
    hipError_t alloc(size_t cap_new) {
        if (cap_new <= cap) return hipSuccess;
        reset();
        void* q = nullptr;
        const hipError_t e = Mem::alloc(&q, cap_new * sizeof(T));
        if (e != hipSuccess) return e;
        p = static_cast<T*>(q); cap = cap_new;
        return hipSuccess;
    }
    hipError_t grow_keep(size_t cap_new, size_t keep, hipStream_t st) {
        if (cap_new <= cap) return hipSuccess;
        void* q = nullptr;
        hipError_t e = Mem::alloc(&q, cap_new * sizeof(T));
        if (e != hipSuccess) return e;
        if (keep > 0 && p) e = Mem::copy(q, p, keep * sizeof(T), st);
        if (e == hipSuccess) e = Mem::sync();             // the copy is done, and nothing reads the old block any more
        if (e != hipSuccess) { (void)Mem::free(q); return e; }
        if (p) (void)Mem::free(p);
        p = static_cast<T*>(q); cap = cap_new;
        return hipSuccess;
    }
};
