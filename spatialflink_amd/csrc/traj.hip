// traj.hip -- the trajectory family's keyBy(objID) on the device, and the two operators it fully
// determines: windowed PointTStatsQuery and windowed / real-time PointTFilterQuery.
//
// Reference (paths relative to the reference's src/main/java/GeoFlink):
//   selection   spatialOperators/tStats/PointTStatsQuery.java:76-84, tFilter/PointTFilterQuery.java:62-73, 89-97:
//               an empty trajIDSet selects every point, otherwise trajIDSet.contains(point.objID)
//               (String.equals = byte equality of the UTF-8 stored here); a null objID is in no set;
//   grouping    keyBy(p -> p.objID).window(..) (PointTStatsQuery.java:86-92, PointTFilterQuery.java:100-107):
//               each key's points reach the window function in arrival order = ascending window index;
//               a null key makes Flink throw -> GEOHIP_ERR_ARG;
//   TStats      spatialOperators/tStats/TStatsQuery.java:148-189 (TStatsQueryWFunction.apply), distance
//               utils/DistanceFunctions.java:60-63 with Math.pow(v, 2) == v * v (oracle/restate.py:362);
//   TFilter     PointTFilterQuery.java:100-118: one coordinate list per key, arrival order.
//
// Output order across keys (unspecified in Flink): trajectory t is the t-th distinct selected objID
// in order of first appearance, so traj_first[t] names its objID.
//
// geohip_traj_group:
//   1. traj_set_build  the selection set's strings into their own open-addressing table;
//   2. traj_insert     per point: 64-bit hash of the objID bytes, selection-set probe, then CAS insert
//                      into a table of >= 2n slots.  A slot holds the index of one point that carries
//                      the slot's string (its representative): every probe compares the full bytes with
//                      the representative's -- a hash only picks the first slot -- and a match lowers
//                      the slot to the smaller index (atomicMin), which stays a representative, so when
//                      the kernel ends the slot holds the string's first appearance;
//      (GEOHIP_TRAJ_NULL_KEY: a null objID takes no slot; the null points lower one word to
//      their smallest index, which is their representative);
//   3. traj_flag + exclusive scan (rocPRIM): dense ids in first-appearance order;
//   4. traj_finalize   traj_of, traj_first and the sort keys (unselected points get key T);
//   5. stable LSD radix sort (rocPRIM) of (traj_of, index) over ceil(log2(T + 1)) bits: perm;
//   6. traj_offsets    run boundaries of the sorted keys: traj_off.
// geohip_tstats: the per-key loop is serial by definition.  Trajectories of up to kSerialMax points
// are walked one per lane (tstats_serial, the loop as written); longer ones are queued and walked one
// per wave, 64 points a step (tstats_wave): the keep / skip decisions from a prefix maximum across
// the lanes, the kept segments' distances in parallel, and their sum lane by lane in ascending order
// -- the same additions in the same order as the loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "geohip.h"
#include "traj_common.h"

namespace geohip {
namespace {

constexpr unsigned long long kOffMask = ~(1ull << 63);

// scratch slots (kCallSlots, traj_common.h)
enum TSlot { T_TAB, T_KEY, T_RANK, T_KEY2, T_VAL, T_VAL2, T_TEMP, T_WORDS, T_SETTAB, T_LIST };

// words block: [0] error bits, [1] selected points, [2] queued long trajectories, [3] the null
// objID's representative (GEOHIP_TRAJ_NULL_KEY: the smallest index of a null point, kNone = none)
constexpr unsigned kNullSlot = 0xfffffffeu;  // traj_of between traj_insert and traj_finalize: the null trajectory (no table slot)
constexpr unsigned kErrNullKey = 1u;   // null objID under an empty set (Flink: null key)
constexpr unsigned kErrOffsets = 2u;   // oid_off / set_off not ascending
constexpr unsigned kErrInternal = 4u;  // a probe walked the whole table
constexpr unsigned kErrIndex = 8u;     // geohip_tstats / _traj_gather: perm entry >= n, or traj_off not ascending or past n_sel

struct Strs {
    const uint8_t* text;
    const unsigned long long* off;
};

// FNV-1a over the bytes, then the splitmix64 finaliser so the low bits (the slot) depend on all of it.
__device__ __forceinline__ uint64_t hash_bytes(const uint8_t* p, uint64_t len) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t k = 0; k < len; k++) h = (h ^ p[k]) * 0x100000001b3ull;
    h = (h ^ (h >> 30)) * 0xbf58476d1ce4e5b9ull;
    h = (h ^ (h >> 27)) * 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}

__device__ __forceinline__ bool bytes_equal(const uint8_t* a, const uint8_t* b, uint64_t len) {
    for (uint64_t k = 0; k < len; k++)
        if (a[k] != b[k]) return false;
    return true;
}

__device__ __forceinline__ bool same_string(const Strs& s, unsigned r, const uint8_t* p, uint64_t len) {
    const uint64_t rb = s.off[r] & kOffMask, re = s.off[r + 1] & kOffMask;
    return re - rb == len && bytes_equal(s.text + rb, p, len);
}

// Insert string i of s (bytes p[0, len), hash h) into tab (slots + 1 = a power of two): the slot
// of its string, or kNone if the table is full (never: it has more slots than strings).
__device__ unsigned table_insert(unsigned* tab, unsigned slots_mask, uint64_t h, const Strs& s, unsigned i,
                                 const uint8_t* p, uint64_t len) {
    unsigned slot = (unsigned)h & slots_mask;
    for (unsigned probe = 0; probe <= slots_mask; probe++, slot = (slot + 1) & slots_mask) {
        unsigned r = __hip_atomic_load(&tab[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (r == kNone) {
            r = atomicCAS(&tab[slot], kNone, i);
            if (r == kNone) return slot;
        }
        // r carries the slot's string for good (only equal strings replace it)
        if (r == i || same_string(s, r, p, len)) {
            if (i < r) atomicMin(&tab[slot], i);
            return slot;
        }
    }
    return kNone;
}

// Is the string p[0, len) (hash h) in the set table?
__device__ bool table_contains(const unsigned* tab, unsigned slots_mask, uint64_t h, const Strs& s, const uint8_t* p,
                               uint64_t len) {
    unsigned slot = (unsigned)h & slots_mask;
    for (unsigned probe = 0; probe <= slots_mask; probe++, slot = (slot + 1) & slots_mask) {
        const unsigned r = tab[slot];
        if (r == kNone) return false;
        if (same_string(s, r, p, len)) return true;
    }
    return false;
}

__global__ void __launch_bounds__(kTB) traj_set_build(Strs set, unsigned s, unsigned* tab, unsigned slots_mask,
                                                      uint64_t hmask, unsigned* words) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= s) return;
    const uint64_t b = set.off[i] & kOffMask, e = set.off[i + 1] & kOffMask;
    if (e < b || (e > b && !set.text)) {
        atomicOr(&words[0], kErrOffsets);
        return;
    }
    const uint8_t* p = set.text + b;
    if (table_insert(tab, slots_mask, hash_bytes(p, e - b) & hmask, set, i, p, e - b) == kNone)
        atomicOr(&words[0], kErrInternal);
}

// traj_of[i] = the table slot of point i's objID, kNone for an unselected point.
__global__ void __launch_bounds__(kTB) traj_insert(Strs oid, unsigned n, Strs set, unsigned s, const unsigned* set_tab,
                                                   unsigned set_mask, unsigned* tab, unsigned slots_mask, uint64_t hmask,
                                                   unsigned null_key, unsigned* traj_of, unsigned* words) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    unsigned slot = kNone;
    if (i < n) {
        const unsigned long long o0 = oid.off[i], o1 = oid.off[i + 1];
        if (o0 >> 63) {
            // PointTStatsQuery.java:76-84: null is in no non-empty set; with an empty set it reaches
            // keyBy as a null key, where Flink throws -- unless the caller keys by something else
            // and keeps the objIDs in a HashMap, which admits the null key (GEOHIP_TRAJ_NULL_KEY)
            if (s == 0) {
                if (null_key) slot = kNullSlot;
                else atomicOr(&words[0], kErrNullKey);
            }
        } else {
            const uint64_t b = o0 & kOffMask, e = o1 & kOffMask;
            if (e < b || (e > b && !oid.text)) {
                atomicOr(&words[0], kErrOffsets);
            } else {
                const uint8_t* p = oid.text + b;
                const uint64_t len = e - b;
                const uint64_t h = hash_bytes(p, len) & hmask;
                if (s == 0 || table_contains(set_tab, set_mask, h, set, p, len)) {
                    slot = table_insert(tab, slots_mask, h, oid, i, p, len);
                    if (slot == kNone) atomicOr(&words[0], kErrInternal);
                }
            }
        }
        traj_of[i] = slot;
    }
    // the null trajectory's representative: indices ascend with the lane, so a wave's lowest null
    // lane holds its smallest, and it writes only while it would lower the word
    const unsigned long long nulls = __ballot(slot == kNullSlot);
    if (nulls && (threadIdx.x & 63u) == (unsigned)(__ffsll((long long)nulls) - 1) &&
        i < __hip_atomic_load(&words[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMin(&words[3], i);
    // the selected count: one add per workgroup (every wave adding to the one word costs more than
    // the rest of the kernel)
    const int c = __syncthreads_count(slot != kNone);
    if (threadIdx.x == 0 && c) atomicAdd(&words[1], (unsigned)c);
}

// flag[i] = point i is its trajectory's first appearance (i <= n; flag[n] = 0 carries the total
// through the exclusive scan).
__global__ void __launch_bounds__(kTB) traj_flag(const unsigned* traj_of, const unsigned* tab, const unsigned* words,
                                                 unsigned n, unsigned* flag) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i > n) return;
    unsigned f = 0;
    if (i < n) {
        const unsigned slot = traj_of[i];
        f = slot != kNone && (slot == kNullSlot ? words[3] : tab[slot]) == i;
    }
    flag[i] = f;
}

__global__ void __launch_bounds__(kTB) traj_finalize(unsigned* traj_of, const unsigned* tab, const unsigned* words,
                                                     const unsigned* rank, unsigned n, unsigned T, unsigned* traj_first,
                                                     unsigned* key, unsigned* val) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const unsigned slot = traj_of[i];
    unsigned k = T;
    if (slot != kNone) {
        const unsigned first = slot == kNullSlot ? words[3] : tab[slot];
        const unsigned t = rank[first];
        traj_of[i] = t;
        if (t < T) {
            k = t;
            if (first == i) traj_first[t] = i;
        }
    }
    key[i] = k;
    val[i] = i;
}

__global__ void __launch_bounds__(kTB) traj_offsets(const unsigned* key, unsigned n_sel, unsigned T, unsigned* traj_off) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    if (j > n_sel) return;
    if (j == n_sel) {
        traj_off[T] = n_sel;
        return;
    }
    const unsigned k = key[j];
    if (k < T && (j == 0 || key[j - 1] != k)) traj_off[k] = j;
}

// real-time TFilter (PointTFilterQuery.java:62-73): the predicate of the selected points' compaction
struct IsSelected {
    const unsigned* traj_of;
    __device__ bool operator()(unsigned i) const { return traj_of[i] != kNone; }
};

// ---- TStats ---------------------------------------------------------------------------------
constexpr unsigned kSerialMax = 32;  // longer trajectories take the wave walk

// TStatsQuery.java:148-189, the loop body for one point.
struct TState {
    long long last = 0;  // lastTimestamp
    long long tlen = 0;  // temporalLength
    double slen = 0.0;   // spatialLength
    double lx = 0.0, ly = 0.0;
};

// DistanceFunctions.java:60-63: Math.sqrt(Math.pow(lat1 - lat, 2) + Math.pow(lon1 - lon, 2))
__device__ __forceinline__ double pp_euclid(double lx, double ly, double x, double y) {
    const double dy = y - ly, dx = x - lx;
    return __builtin_sqrt(dy * dy + dx * dx);
}

__device__ __forceinline__ void tstats_emit(const TState& st, unsigned t, double* out_s, long long* out_t, double* out_avg) {
    out_s[t] = st.slen;
    out_t[t] = st.tlen;
    out_avg[t] = st.slen / (double)st.tlen;  // Double / Long: 0.0 / 0 = NaN, S / 0 = +-Infinity
}

__global__ void __launch_bounds__(kTB) tstats_serial(const double* x, const double* y, const long long* ts, unsigned n,
                                                     const unsigned* perm, unsigned n_sel, const unsigned* traj_off,
                                                     unsigned T, double* out_s, long long* out_t, double* out_avg, unsigned* list,
                                                     unsigned* words) {
    const unsigned t = blockIdx.x * kTB + threadIdx.x;
    if (t >= T) return;
    const unsigned b = traj_off[t], e = traj_off[t + 1];
    if (e < b || e > n_sel) {
        atomicOr(&words[0], kErrIndex);
        return;
    }
    if (e - b > kSerialMax) {
        list[atomicAdd(&words[2], 1u)] = t;
        return;
    }
    TState st;
    for (unsigned j = b; j < e; j++) {
        const unsigned p = perm[j];
        if (p >= n) {
            atomicOr(&words[0], kErrIndex);
            return;
        }
        const long long tp = ts[p];
        if (st.last == 0) {  // "first point" is a test of the value (TStatsQuery.java:164)
            st.last = tp;
            st.lx = x[p];
            st.ly = y[p];
            st.slen = 0.0;
            st.tlen = 0;
        } else if (tp > st.last) {
            const double px = x[p], py = y[p];
            st.slen += pp_euclid(st.lx, st.ly, px, py);
            st.tlen = (long long)((unsigned long long)st.tlen + ((unsigned long long)tp - (unsigned long long)st.last));
            st.last = tp;
            st.lx = px;
            st.ly = py;
        }
    }
    tstats_emit(st, t, out_s, out_t, out_avg);
}

// One wave per trajectory, 64 points a step, no re-initialisation inside the walk.  The loop of
// TStatsQuery.java:157-187 re-initialises exactly when lastTimestamp is 0 as a point arrives, and
// lastTimestamp is the largest timestamp since the last (re-)initialisation.  So with P = the first
// point with ts > 0 (from there on lastTimestamp stays positive) every ts == 0 point before P makes
// its successor re-initialise, and nothing else does: the result is that of the points from s =
// (the last zero before P that has a successor) + 1 on, walked with no re-initialisation --
//   kept(j) = j == s or ts[j] > max(ts[s .. j-1]),  S = the kept points' segment lengths added in
//   order,  T = ts[last kept] - ts[s] mod 2^64 (the sum of the kept differences telescopes).
// Pass 1 finds s with ballots; pass 2 takes 64 points a step: prefix maximum of ts across the lanes
// (seeded with the running maximum), each kept lane's predecessor = the highest kept lane below it
// (else the carried point), the distances in parallel, then S += d lane by lane in ascending order.
constexpr long long kLongMin = (long long)(1ull << 63);

__global__ void __launch_bounds__(kTB) tstats_wave(const double* x, const double* y, const long long* ts, unsigned n,
                                                   const unsigned* perm, const unsigned* traj_off, const unsigned* list,
                                                   double* out_s, long long* out_t, double* out_avg, unsigned* words) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long lanes_below = (1ull << lane) - 1;
    const unsigned count = words[2];
    for (unsigned q = blockIdx.x * (kTB / 64) + wave; q < count; q += gridDim.x * (kTB / 64)) {
        const unsigned t = list[q];
        const unsigned b = traj_off[t], e = traj_off[t + 1];  // tstats_serial checked b < e <= n_sel
        bool bad = false;
        unsigned z1 = kNone, z2 = kNone;  // the last two ts == 0 points before P
        for (unsigned c = b; c < e; c += 64) {
            const unsigned j = c + lane;
            long long tp = -1;  // past the end: neither zero nor positive
            bool oob = false;
            if (j < e) {
                const unsigned p = perm[j];
                if (p < n)
                    tp = ts[p];
                else
                    oob = true;
            }
            if (__ballot(oob)) {
                bad = true;
                break;
            }
            const unsigned long long pos = __ballot(tp > 0);
            unsigned long long zero = __ballot(tp == 0);
            if (pos) zero &= (1ull << (__ffsll((long long)pos) - 1)) - 1;
            if (zero) {
                const int h = 63 - __clzll((long long)zero);
                z2 = z1;
                z1 = c + h;
                zero &= ~(1ull << h);
                if (zero) z2 = c + (63 - __clzll((long long)zero));
            }
            if (pos) break;
        }
        if (z1 != kNone && z1 == e - 1) z1 = z2;  // a zero that ends the trajectory has no successor
        const unsigned s = z1 != kNone ? z1 + 1 : b;
        long long last = 0, first_ts = 0;
        double lx = 0.0, ly = 0.0, slen = 0.0;
        bool have = false;
        for (unsigned c = s; c < e && !bad; c += 64) {
            const unsigned j = c + lane;
            const bool valid = j < e;
            long long tp = kLongMin;
            double px = 0.0, py = 0.0;
            bool oob = false;
            if (valid) {
                const unsigned p = perm[j];
                if (p < n) {
                    tp = ts[p];
                    px = x[p];
                    py = y[p];
                } else {
                    oob = true;
                }
            }
            if (__ballot(oob)) {
                bad = true;
                break;
            }
            long long inc = tp;  // inclusive prefix maximum over the lanes
            for (int d = 1; d < 64; d <<= 1) {
                const long long o = __shfl_up(inc, d);
                if ((int)lane >= d && o > inc) inc = o;
            }
            long long exc = __shfl_up(inc, 1);
            if (lane == 0) exc = have ? last : kLongMin;
            if (have && last > exc) exc = last;
            const bool keep = valid && ((!have && lane == 0) || tp > exc);
            const unsigned long long km = __ballot(keep);  // bit 0 is set in the first step (the point s)
            const unsigned long long below = km & lanes_below;
            const int src = below ? 63 - __clzll((long long)below) : (int)lane;
            double qx = __shfl(px, src), qy = __shfl(py, src);
            if (!below) {
                qx = lx;
                qy = ly;
            }
            const double d = pp_euclid(qx, qy, px, py);
            unsigned long long dm = have ? km : km & ~1ull;  // the point s starts the walk: no segment
            while (dm) {
                slen += __shfl(d, __ffsll((long long)dm) - 1);
                dm &= dm - 1;
            }
            if (!have) first_ts = __shfl(tp, 0);
            if (km) {
                const int h = 63 - __clzll((long long)km);
                last = __shfl(tp, h);
                lx = __shfl(px, h);
                ly = __shfl(py, h);
            }
            have = true;
        }
        if (lane == 0) {
            if (bad) {
                atomicOr(&words[0], kErrIndex);
            } else {
                TState st;
                st.slen = slen;
                st.tlen = (long long)((unsigned long long)last - (unsigned long long)first_ts);
                tstats_emit(st, t, out_s, out_t, out_avg);
            }
        }
    }
}

__global__ void __launch_bounds__(kTB) traj_gather(const double* x, const double* y, const long long* ts, unsigned n,
                                                   const unsigned* perm, unsigned m, double* out_x, double* out_y,
                                                   long long* out_ts, unsigned* words) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    if (j >= m) return;
    const unsigned p = perm[j];
    if (p >= n) {
        atomicOr(&words[0], kErrIndex);
        return;
    }
    out_x[j] = x[p];
    out_y[j] = y[p];
    if (ts) out_ts[j] = ts[p];
}

// ---- host side --------------------------------------------------------------------------------
// slots - 1 of a table for n strings: a power of two >= max(2n, 64)
unsigned table_mask(uint64_t n) {
    uint64_t m = 64;
    while (m < 2 * n) m <<= 1;
    return (unsigned)(m - 1);
}

int traj_group_impl(geohip_ctx* ctx, const uint8_t* oid_text, const uint64_t* oid_off, uint64_t n,
                    const uint8_t* set_text, const uint64_t* set_off, uint64_t s, uint64_t hmask, uint32_t flags, uint32_t* traj_of,
                    uint32_t* traj_first, uint32_t* traj_off, uint32_t* perm, uint64_t cap_traj, uint64_t* n_traj,
                    uint64_t* n_sel) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!n_traj || !n_sel) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null n_traj / n_sel");
    *n_traj = 0;
    *n_sel = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_traj_group takes device memory");
    if (flags & ~(uint32_t)GEOHIP_TRAJ_NULL_KEY) return ctx_fail(ctx, GEOHIP_ERR_ARG, "unknown flag");
    if (n > kMaxPoints || s > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points or set entries");
    if (!traj_off || (n && (!oid_off || !traj_of || !perm)) || (s && !set_off))
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    if (n == 0) {
        GEOHIP_CHK(hipMemsetAsync(traj_off, 0, 4, st));
        return GEOHIP_OK;
    }
    const unsigned nn = (unsigned)n, ss = (unsigned)s;
    const unsigned mask = table_mask(n), set_mask = table_mask(s);
    size_t scan_tb = 0, sort_tb = 0;
    GEOHIP_CHK(rocprim::exclusive_scan(nullptr, scan_tb, (unsigned*)nullptr, (unsigned*)nullptr, 0u, n + 1,
                                       rocprim::plus<unsigned>(), st));
    GEOHIP_CHK(rocprim::radix_sort_pairs(nullptr, sort_tb, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                         (unsigned*)nullptr, n, 0, 32, st));
    const size_t temp_bytes = (scan_tb > sort_tb ? scan_tb : sort_tb) + 16;
    unsigned *tab, *key, *rank, *key2, *val, *val2, *words, *set_tab;
    void* temp;
    rc = scratch<T_TAB>(ctx, ((size_t)mask + 1) * 4, &tab);
    if (!rc) rc = scratch<T_KEY>(ctx, (n + 1) * 4, &key);
    if (!rc) rc = scratch<T_RANK>(ctx, (n + 1) * 4, &rank);
    if (!rc) rc = scratch<T_KEY2>(ctx, n * 4, &key2);
    if (!rc) rc = scratch<T_VAL>(ctx, n * 4, &val);
    if (!rc) rc = scratch<T_VAL2>(ctx, n * 4, &val2);
    if (!rc) rc = scratch<T_TEMP>(ctx, temp_bytes, &temp);
    if (!rc) rc = scratch<T_WORDS>(ctx, 64, &words);
    if (!rc) rc = scratch<T_SETTAB>(ctx, ((size_t)set_mask + 1) * 4, &set_tab);
    if (rc) return rc;
    const Strs oid{oid_text, reinterpret_cast<const unsigned long long*>(oid_off)};
    const Strs set{set_text, reinterpret_cast<const unsigned long long*>(set_off)};
    GEOHIP_CHK(hipMemsetAsync(tab, 0xff, ((size_t)mask + 1) * 4, st));
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    GEOHIP_CHK(hipMemsetAsync(words + 3, 0xff, 4, st));
    if (ss) {
        GEOHIP_CHK(hipMemsetAsync(set_tab, 0xff, ((size_t)set_mask + 1) * 4, st));
        tlaunch(ctx, traj_set_build, dim3(blocks_for(s)), dim3(kTB), 0, st, set, ss, set_tab, set_mask, hmask, words);
    }
    tlaunch(ctx, traj_insert, dim3(blocks_for(n)), dim3(kTB), 0, st, oid, nn, set, ss, set_tab, set_mask, tab, mask, hmask,
            (unsigned)(flags & GEOHIP_TRAJ_NULL_KEY), traj_of, words);
    unsigned* flag = key;  // dead once scanned
    tlaunch(ctx, traj_flag, dim3(blocks_for(n + 1)), dim3(kTB), 0, st, traj_of, tab, (const unsigned*)words, nn, flag);
    size_t tb = temp_bytes;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb, flag, rank, 0u, n + 1, rocprim::plus<unsigned>(), st));
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 8, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipMemcpyAsync(pin + 1, rank + n, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    const unsigned err = (unsigned)(pin[0] & 0xffffffffu);
    const unsigned nsel = (unsigned)(pin[0] >> 32), T = (unsigned)(pin[1] & 0xffffffffu);
    if (err & kErrOffsets) return ctx_fail(ctx, GEOHIP_ERR_ARG, "oid_off / set_off is not ascending (or names bytes of a null text)");
    if (err & kErrInternal) return ctx_fail(ctx, GEOHIP_ERR_DEVICE, "internal: objID table full");
    if (err & kErrNullKey)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "a null objID with an empty trajIDSet (keyBy of a null key throws)");
    *n_traj = T;
    *n_sel = nsel;
    if (T > cap_traj) return ctx_fail(ctx, GEOHIP_ERR_CAPACITY, "cap_traj too small; *n_traj = required");
    if (T && !traj_first) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null traj_first");
    tlaunch(ctx, traj_finalize, dim3(blocks_for(n)), dim3(kTB), 0, st, traj_of, tab, (const unsigned*)words, rank, nn, T, traj_first,
            key, val);
    const unsigned bits = std::max(1u, bits_for((uint64_t)T + 1));  // keys 0..T
    unsigned* sorted = nsel == nn ? perm : val2;
    tb = temp_bytes;
    GEOHIP_CHK(rocprim::radix_sort_pairs(temp, tb, (const unsigned*)key, key2, (const unsigned*)val, sorted, n, 0, bits, st));
    if (sorted != perm && nsel) GEOHIP_CHK(hipMemcpyAsync(perm, sorted, (size_t)nsel * 4, hipMemcpyDeviceToDevice, st));
    tlaunch(ctx, traj_offsets, dim3(blocks_for((uint64_t)nsel + 1)), dim3(kTB), 0, st, key2, nsel, T, traj_off);
    GEOHIP_CHK(hipGetLastError());
    return GEOHIP_OK;
}

// the words block's error bits after the queued work (geohip_tstats, geohip_traj_gather)
int index_check(geohip_ctx* ctx, unsigned* words, hipStream_t st, const char* what) {
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipGetLastError());
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 8, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    if (pin[0] & kErrIndex) return ctx_fail(ctx, GEOHIP_ERR_ARG, std::string(what) + ": perm entry >= n, or traj_off not ascending or past n_sel");
    return GEOHIP_OK;
}

}  // namespace
}  // namespace geohip

using namespace geohip;

extern "C" {

int geohip_traj_group(geohip_ctx* ctx, const uint8_t* oid_text, const uint64_t* oid_off, uint64_t n,
                      const uint8_t* set_text, const uint64_t* set_off, uint64_t s, uint32_t* traj_of,
                      uint32_t* traj_first, uint32_t* traj_off, uint32_t* perm, uint64_t cap_traj, uint64_t* n_traj,
                      uint64_t* n_sel) {
    return traj_group_impl(ctx, oid_text, oid_off, n, set_text, set_off, s, ~0ull, 0, traj_of, traj_first, traj_off, perm,
                           cap_traj, n_traj, n_sel);
}

int geohip_traj_group_flags(geohip_ctx* ctx, const uint8_t* oid_text, const uint64_t* oid_off, uint64_t n,
                            const uint8_t* set_text, const uint64_t* set_off, uint64_t s, uint32_t* traj_of,
                            uint32_t* traj_first, uint32_t* traj_off, uint32_t* perm, uint64_t cap_traj, uint64_t* n_traj,
                            uint64_t* n_sel, uint32_t flags) {
    return traj_group_impl(ctx, oid_text, oid_off, n, set_text, set_off, s, ~0ull, flags, traj_of, traj_first, traj_off, perm,
                           cap_traj, n_traj, n_sel);
}

// Test hook: geohip_traj_group with every hash ANDed with hash_mask before probing (0: all strings
// collide in one chain, 3: four chains), so the byte-compare and probe-chain paths run whatever
// the hash function is.  The result is geohip_traj_group's.
int geohip_debug_traj_group_masked(geohip_ctx* ctx, uint64_t hash_mask, const uint8_t* oid_text, const uint64_t* oid_off,
                                   uint64_t n, const uint8_t* set_text, const uint64_t* set_off, uint64_t s,
                                   uint32_t* traj_of, uint32_t* traj_first, uint32_t* traj_off, uint32_t* perm,
                                   uint64_t cap_traj, uint64_t* n_traj, uint64_t* n_sel) {
    return traj_group_impl(ctx, oid_text, oid_off, n, set_text, set_off, s, hash_mask, 0, traj_of, traj_first, traj_off, perm,
                           cap_traj, n_traj, n_sel);
}

int geohip_tstats(geohip_ctx* ctx, const double* x, const double* y, const int64_t* ts, uint64_t n, const uint32_t* perm,
                  uint64_t n_sel, const uint32_t* traj_off, uint64_t n_traj, double* out_spatial, int64_t* out_temporal, double* out_avg) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tstats takes device memory");
    if (n > kMaxPoints || n_sel > kMaxPoints || n_traj > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (n_traj == 0) return GEOHIP_OK;
    if (!x || !y || !ts || !perm || !traj_off || !out_spatial || !out_temporal || !out_avg)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    const unsigned T = (unsigned)n_traj;
    unsigned *words, *list;
    rc = scratch<T_WORDS>(ctx, 64, &words);
    if (!rc) rc = scratch<T_LIST>(ctx, (size_t)T * 4, &list);
    if (rc) return rc;
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    const long long* lts = reinterpret_cast<const long long*>(ts);
    long long* lot = reinterpret_cast<long long*>(out_temporal);
    tlaunch(ctx, tstats_serial, dim3(blocks_for(T)), dim3(kTB), 0, st, x, y, lts, (unsigned)n, perm, (unsigned)n_sel, traj_off,
            T, out_spatial, lot, out_avg, list, words);
    // the queue's length stays on the device: a fixed grid of waves strides over it
    const unsigned want = (T + kTB / 64 - 1) / (kTB / 64);
    const unsigned grid = want < 8192u ? want : 8192u;
    tlaunch(ctx, tstats_wave, dim3(grid), dim3(kTB), 0, st, x, y, lts, (unsigned)n, perm, traj_off, (const unsigned*)list,
            out_spatial, lot, out_avg, words);
    return index_check(ctx, words, st, "geohip_tstats");
}

int geohip_traj_gather(geohip_ctx* ctx, const double* x, const double* y, const int64_t* ts, uint64_t n,
                       const uint32_t* perm, uint64_t m, double* out_x, double* out_y, int64_t* out_ts) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_traj_gather takes device memory");
    if (n > kMaxPoints || m > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (m == 0) return GEOHIP_OK;
    if (!x || !y || !perm || !out_x || !out_y || (ts && !out_ts)) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    unsigned* words;
    rc = scratch<T_WORDS>(ctx, 64, &words);
    if (rc) return rc;
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    tlaunch(ctx, traj_gather, dim3(blocks_for(m)), dim3(kTB), 0, st, x, y, reinterpret_cast<const long long*>(ts),
            (unsigned)n, perm, (unsigned)m, out_x, out_y, reinterpret_cast<long long*>(out_ts), words);
    return index_check(ctx, words, st, "geohip_traj_gather");
}

int geohip_traj_selected(geohip_ctx* ctx, const uint32_t* traj_of, uint64_t n, uint32_t* out_idx, uint64_t* out_count) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!out_count) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out_count");
    *out_count = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_traj_selected takes device memory");
    if (n > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (n == 0) return GEOHIP_OK;
    if (!traj_of || !out_idx) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    const rocprim::counting_iterator<unsigned> iota(0u);
    const IsSelected pred{traj_of};
    size_t tb = 0;
    GEOHIP_CHK(rocprim::select(nullptr, tb, iota, out_idx, (unsigned*)nullptr, n, pred, st));
    unsigned* words;
    void* temp;
    rc = scratch<T_WORDS>(ctx, 64, &words);
    if (!rc) rc = scratch<T_TEMP>(ctx, tb + 16, &temp);
    if (rc) return rc;
    GEOHIP_CHK(rocprim::select(temp, tb, iota, out_idx, words, n, pred, st));
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    *out_count = pin[0] & 0xffffffffu;
    return GEOHIP_OK;
}

}  // extern "C"
