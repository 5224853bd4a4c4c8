// traj_common.h -- what the trajectory sources (traj.hip, trange.hip, tagg.hip, tjoin.hip) share:
// the launch constants, the per-call scratch slots, the words-block read-back and the wave and
// workgroup reductions of the locate kernels.  Only those four include it: cell_kernels.hip has a
// geohip::kTB of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "join.h"
#include "locate.h"

namespace geohip {

constexpr int kTB = 256;  // threads per workgroup of every trajectory kernel
constexpr int kWaves = kTB / 64;
constexpr unsigned kNone = 0xffffffffu;
// geohip_traj_group's bound on points and trajectories: table slots (<= 2^31) and indices stay
// below kNone, and a trajectory id leaves the top bits of a u64 key clear
constexpr uint64_t kMaxPoints = 1ull << 30;

// Scratch slots (ctx_ensure): a trajectory call owns slots 0 .. kCallSlots - 1 for its own duration
// on the ctx stream and carries nothing in them from one call to the next, so the trajectory calls
// may share them.  The slots from kCallSlots up are not theirs: the point and polygon queries keep
// state there between calls (slot 10 holds the point-polygon join's uploaded polygon tables,
// cell_kernels.hip J_POLY), which a trajectory call in between must leave alone.
constexpr int kCallSlots = 10;

template <int SLOT, typename T>
int scratch(geohip_ctx* ctx, size_t bytes, T** out) {
    static_assert(SLOT >= 0 && SLOT < kCallSlots, "a scratch slot that no call keeps state in");
    void* p = nullptr;
    const int rc = ctx_ensure(ctx, SLOT, bytes, &p);
    *out = static_cast<T*>(p);
    return rc;
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + kTB - 1) / kTB); }

inline unsigned bits_for(uint64_t span) {  // bits that hold 0 .. span - 1
    unsigned b = 0;
    while (b < 63 && (1ull << b) < span) b++;
    return b;
}

inline uint64_t pow2_at_least(uint64_t v) {  // at least 2
    uint64_t p = 2;
    while (p < v) p <<= 1;
    return p;
}

// The head of a words block as locate_reduce leaves it: [0] error bits, [1] a count, [2..5] four
// maxima.  What the count and the maxima mean is the caller's.
struct WordsHead {
    unsigned err, count, hx, lx, hy, ly;
};

// The launches so far, then the head of the words block through the pinned buffer (synchronises).
inline int read_words_head(geohip_ctx* ctx, const unsigned* words, hipStream_t st, WordsHead* h) {
    GEOHIP_CHK(hipGetLastError());
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 24, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    *h = WordsHead{(unsigned)(pin[0] & 0xffffffffu), (unsigned)(pin[0] >> 32), (unsigned)(pin[1] & 0xffffffffu),
                   (unsigned)(pin[1] >> 32),         (unsigned)(pin[2] & 0xffffffffu), (unsigned)(pin[2] >> 32)};
    return GEOHIP_OK;
}

__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// first j in [0, n) with key[j] >= k (n where none)
__device__ __forceinline__ unsigned lower_bound(const unsigned* key, unsigned n, unsigned k) {
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + (hi - lo) / 2;
        if (key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The end of a locate kernel (kTB threads, all of them here): a wave's error flag and count
// (wave-uniform) and every thread's four maxima go through LDS to thread 0, which issues the
// workgroup's one set of atomics: err_bit into words[0], the count added to words[1], the maxima
// into words[2..5].  Zero is the identity of all six, so a zero issues nothing.
__device__ __forceinline__ void locate_reduce(unsigned werr, unsigned wcount, unsigned hx, unsigned lx, unsigned hy,
                                              unsigned ly, unsigned err_bit, unsigned* words) {
    __shared__ unsigned red[kWaves][6];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    hx = wave_max(hx);
    lx = wave_max(lx);
    hy = wave_max(hy);
    ly = wave_max(ly);
    if (lane == 0) {
        red[wave][0] = werr;
        red[wave][1] = wcount;
        red[wave][2] = hx;
        red[wave][3] = lx;
        red[wave][4] = hy;
        red[wave][5] = ly;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned a[6] = {0, 0, 0, 0, 0, 0};
        for (int w = 0; w < kWaves; w++) {
            a[0] |= red[w][0];
            a[1] += red[w][1];
            for (int k = 2; k < 6; k++) a[k] = red[w][k] > a[k] ? red[w][k] : a[k];
        }
        if (a[0]) atomicOr(&words[0], err_bit);
        if (a[1]) atomicAdd(&words[1], a[1]);
        for (int k = 2; k < 6; k++)
            if (a[k]) atomicMax(&words[k], a[k]);
    }
}

}  // namespace geohip
