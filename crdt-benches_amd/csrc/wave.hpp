// wave.hpp — wave64 / workgroup primitives shared by the gfx950 kernels (every .hip file), and
// what their host sides share: device memory, and the scratch of one call (CallScratch: transient
// arrays, counters with their pinned copy, the event pair that times the kernels).  Header-only,
// internal linkage.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "util.hpp"

namespace crdt {
namespace {

template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp_add(uint32_t x) {
    return x + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROWMASK, 0xf, false);
}
// Inclusive wave64 prefix sum with DPP: row_shr 1,2,4,8 inside 16-lane rows, then
// row_bcast:15 and row_bcast:31 carry across rows (GFX9 DPP, valid on gfx950).
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
    x = dpp_add<0x111, 0xf>(x);
    x = dpp_add<0x112, 0xf>(x);
    x = dpp_add<0x114, 0xf>(x);
    x = dpp_add<0x118, 0xf>(x);
    x = dpp_add<0x142, 0xa>(x);
    x = dpp_add<0x143, 0xc>(x);
    return x;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan(x), 63);
}

// Exclusive scan over the block's threads (NW waves); returns the block total in `total`.
template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* lds, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = wave_incl_scan(x);
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        uint32_t t = lds[i];
        off += (i < (int)w) ? t : 0u;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return off + inc - x;
}

// One workgroup of NT threads: the counts in[0..m) -> their exclusive prefixes out[0..m) (out may
// be in), in rounds of NT with the carry of the rounds before; returns the total in every thread.
// lds: NT / 64 entries.  A prefix is stored as u32: a caller whose total may pass 2^32 compares the
// returned one.
template <int NT>
__device__ __forceinline__ uint64_t block_scan_counts(const uint32_t* in, uint32_t* out, uint32_t m,
                                                      uint32_t* lds) {
    uint64_t c = 0;
    for (uint32_t base = 0; base < m; base += NT) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t x = i < m ? in[i] : 0u;
        uint32_t t;
        const uint32_t e = block_excl_scan<NT / 64>(x, lds, t);
        if (i < m) out[i] = (uint32_t)c + e;
        c += t;
    }
    return c;
}
template <int NT>
__device__ __forceinline__ uint64_t block_scan_counts(uint32_t* v, uint32_t m, uint32_t* lds) {
    return block_scan_counts<NT>(v, v, m, lds);
}

// Sum of x over the block's threads (NW waves), valid in thread 0 (a device-wide counter then
// takes one atomic per block: thousands of same-address atomics, one per wave, serialise at the
// L2 and cost more than the kernels that count with them).
template <int NW>
__device__ __forceinline__ uint32_t block_sum_t0(uint32_t x, uint32_t* lds) {
    x = wave_sum(x);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = x;
    __syncthreads();
    uint32_t t = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < NW; ++i) t += lds[i];
    __syncthreads();
    return t;
}

__device__ __forceinline__ uint32_t utf8_len(uint32_t c) {
    return c < 0x80u ? 1u : c < 0x800u ? 2u : c < 0x10000u ? 3u : 4u;
}

// The last index in [0, n) whose key is at most v (n: none); key(i) ascends.
template <class V, class K>
__device__ __forceinline__ uint32_t last_at_most(uint32_t n, V v, K&& key) {
    if (n == 0 || key(0) > v) return n;
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (key(mid) <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- device memory (host side) ----
template <class T>
hipError_t dalloc(T** p, uint64_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    return pool_alloc(reinterpret_cast<void**>(p), count * sizeof(T));
}
template <class T>
void dfree(T*& p) {
    pool_free(p);
    p = nullptr;
}
inline uint32_t grid_for(uint64_t n, uint32_t block = 256) {
    return (uint32_t)((n + block - 1) / block);
}

// One call's transient device arrays, its counters and the events around its kernels, released
// after a wait for the stream.
struct CallScratch {
    hipStream_t stream;
    std::vector<void*> dev;
    uint64_t* ctl = nullptr;   // device counters
    uint64_t* hctl = nullptr;  // pinned host copy
    hipEvent_t ev[2] = {nullptr, nullptr};  // around each group of kernels
    uint64_t dev_ns = 0;                    // their summed device time
    explicit CallScratch(hipStream_t s) : stream(s) {}
    CallScratch(const CallScratch&) = delete;
    CallScratch& operator=(const CallScratch&) = delete;
    template <class T>
    hipError_t alloc(T** p, uint64_t count) {
        const hipError_t rc = dalloc(p, count);
        if (rc == hipSuccess) dev.push_back(*p);
        return rc;
    }
    hipError_t counters(uint32_t n) {
        hipError_t rc = dalloc(&ctl, (uint64_t)n);
        if (rc == hipSuccess) rc = pool_alloc(reinterpret_cast<void**>(&hctl), n * 8ull, true);
        return rc;
    }
    // Frees the arrays (the caller has waited for the stream); the counters stay.
    void drop_arrays() {
        for (void* p : dev) pool_free(p, false, true);
        dev.clear();
    }
    hipError_t time_begin() {
        for (hipEvent_t& e : ev)
            if (!e) {
                const hipError_t rc = hipEventCreate(&e);
                if (rc != hipSuccess) return rc;
            }
        return hipEventRecord(ev[0], stream);
    }
    hipError_t time_end() { return hipEventRecord(ev[1], stream); }
    void time_add() {  // (after a wait for the stream)
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) dev_ns += (uint64_t)(ms * 1e6);
    }
    ~CallScratch() {
        (void)hipStreamSynchronize(stream);
        drop_arrays();
        if (ctl) pool_free(ctl, false, true);
        if (hctl) pool_free(hctl, true);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

}  // namespace
}  // namespace crdt
