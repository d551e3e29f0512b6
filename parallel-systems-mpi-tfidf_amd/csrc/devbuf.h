/*
 * devbuf.h — the engine's device memory: the counted allocator (engine.cpp) and DevBuf, the
 * buffer that owns what it holds.  Private to csrc/ (engine_ctx.h and group.cpp include it).
 */
#ifndef TFIDF_DEVBUF_H
#define TFIDF_DEVBUF_H

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <utility>

/* engine.cpp: hipMalloc counted in tfidf_run_info.device_allocs / device_alloc_bytes, and the
 * hipFree of such memory (`bytes` as allocated), counted beside them: tfidf_alloc_live is the
 * difference.  Every device allocation of the engine goes through this pair. */
hipError_t tfidf_dev_malloc(void** p, size_t bytes);
void tfidf_dev_free(void* p, size_t bytes);

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {   /* by exchange (std::swap: prune, reweight): o's destructor releases ours */
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    int ensure(size_t bytes) {
        if (bytes <= cap && p) return 0;
        const bool regrow = p != nullptr;
        release();
        /* 1/8 headroom (at least 4 KiB) on the first allocation, 1/2 on a regrowth: sizes
         * that vary from run to run (the record totals after K1's overflow records, the
         * partial-record sort buffers: K1's overflow mode depends on the order in which
         * workgroups claim LDS entries) must not reallocate in steady state — hipFree
         * synchronises the device and a 1 GB hipMalloc inside a stage left the GPU idle for
         * ~0.7 ms (the bench counts allocations in its timed steps).  Near the HBM capacity
         * the headroom is dropped rather than failing a size that fits exactly. */
        const size_t head = regrow ? bytes / 2 : bytes / 8;
        const size_t want = bytes < 256 ? 256 : bytes + (head > 4096 ? head : 4096);
        if (exact(want) == 0) return 0;
        return want != bytes ? exact(bytes) : -1;
    }
    /* exactly `bytes`, the contents dropped: no headroom (ensure's two attempts, prune's spares,
     * the transports' staging, the HBM probe) */
    int exact(size_t bytes) {
        release();
        if (tfidf_dev_malloc(&p, bytes) == hipSuccess) { cap = bytes; return 0; }
        (void)hipGetLastError();
        p = nullptr;
        return -1;
    }
    /* grow preserving the first `keep` bytes */
    int grow_keep(size_t bytes, size_t keep, hipStream_t s) {
        if (bytes <= cap && p) return 0;
        DevBuf q;
        if (tfidf_dev_malloc(&q.p, bytes) != hipSuccess) { q.p = nullptr; return -1; }
        q.cap = bytes;
        if (p && keep) {
            if (hipMemcpyAsync(q.p, p, keep, hipMemcpyDeviceToDevice, s) != hipSuccess) return -1;
            if (hipStreamSynchronize(s) != hipSuccess) return -1;
        }
        *this = std::move(q);
        return 0;
    }
    void release() {
        if (p) tfidf_dev_free(p, cap);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T* as() const { return (T*)p; }
};

#endif
