// tagg.hip -- the per-cell trajectory aggregate PointTAggregateQuery (window form) on the device:
// geohip_tagg_cells.
//
// Reference (paths relative to the reference's src/main/java/GeoFlink):
//   window form  spatialOperators/tAggregate/PointTAggregateQuery.java:63-99: keyBy(p.gridID), then
//                TAggregateQuery.java:514-613 (TimeWindowProcessFunction.process; the count window's
//                :397-493 is the same loop): per cell, over its points in arrival order, per objID
//                min / max timestamp and len = max - min (a Java long: wraps), the running sum of
//                the lens, and the strict extremes of every non-first point's len with the objID of
//                the point that set them;
//   cell key     utils/HelperClass.java:104-120: "%05d%05d" of the unclipped indices; compared here as
//                integer pairs, which is the same while every index lies in [-9999, 99999].
//
// The loop's result does not depend on how the cell's points interleave across objIDs: with the
// cell's points of one objID (a run) in arrival order, L_i = wrap(prefix max - prefix min) at every
// point but the run's first; len = the run's last L_i (0 for a one-point run); sum = the lens added
// mod 2^64; MIN = the smallest (L_i, window index i) with L_i < Long.MAX_VALUE, MAX = the largest
// L_i > Long.MIN_VALUE and among its points the smallest window index.
//
// Kernels (kChunk = 256 elements = one workgroup; in the kernels of this file no workgroup waits for
// another -- rocPRIM's device scan, steps 5 and 7, has its own look-back between workgroups):
//   1. tagg_locate     per selected point (perm order) its cell (d_axis_cell), the input checks, the
//                      count of cells outside [-9999, 99999] and the window's cell rectangle (one set
//                      of atomics per workgroup);
//   2. tagg_keys       key = (cx - cx0) << bits(H) | (cy - cy0), u32 (u64 above 32 bits);
//   3. rocPRIM stable LSD radix sort of (key, perm) over the rectangle's bits: perm is ordered by
//                      (trajectory, index), so the result is ordered by (cell, trajectory, index);
//   4. tagg_partials   per chunk: ts and trajectory gathered into sorted streams, run and cell head
//                      counts and the chunk's aggregate of the segmented (min ts, max ts) scan along
//                      runs (wave64 shuffles, then the four waves through LDS);
//   5. rocPRIM exclusive scan of the chunk aggregates (segmented operator + the two counts);
//   6. tagg_apply      per element L_i with the carry of 5; visits at run ends; per chunk a segmented
//                      scan of the cell aggregate (count, sum, both extremes); a cell that starts in
//                      the chunk and ends in it is written at once, the chunk's open leading cell and
//                      the chunk aggregate go to 7 / 8;
//   7. rocPRIM exclusive scan of the chunks' cell aggregates;
//   8. tagg_fix        one thread per chunk: the cell that ends in the chunk but started before it.
// All arithmetic is integer but the AVG division: the results do not depend on execution order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "geohip.h"
#include "traj_common.h"

namespace geohip {
namespace {

constexpr unsigned kChunk = kTB;  // elements per workgroup of the two scans (tests/test_gpu_tagg.py: CHUNK)
constexpr int32_t kCellLo = -9999, kCellHi = 99999;  // 5 + 5 characters of "%05d%05d" split uniquely
constexpr long long kLongMax = 0x7fffffffffffffffLL;
constexpr long long kLongMin = -kLongMax - 1;

// scratch slots (kCallSlots, traj_common.h).  G_PARTS packs the five per-chunk arrays of the two scans.
enum GSlot { G_CXY, G_KEY, G_KEY2, G_VAL2, G_TS, G_TR, G_TEMP, G_WORDS, G_PARTS };

// words block: [0] error bits, [1] points whose cell leaves [kCellLo, kCellHi], [2..5] the cell
// rectangle as maxima of cx - kCellLo, kCellHi - cx, cy - kCellLo, kCellHi - cy, [6] cells, [7] visits
constexpr unsigned kErrIndex = 1u;  // perm entry >= n, or traj_of[perm[j]] >= n_traj

// ---- the two segmented scans' values ---------------------------------------------------------
struct RunV {  // prefix (min, max) of ts along a run
    long long mn, mx;
    static __host__ __device__ RunV identity() { return RunV{kLongMax, kLongMin}; }
    static __host__ __device__ RunV merge(const RunV& a, const RunV& b) {
        return RunV{b.mn < a.mn ? b.mn : a.mn, b.mx > a.mx ? b.mx : a.mx};
    }
};

struct CellV {  // a cell's aggregate over a span of its points, in arrival-free form
    long long sum, min_len, max_len;
    unsigned count, min_pt, max_pt;
    unsigned flag;  // stored forms only: the span holds a cell head (scan input), the entry is set (open)
    static __host__ __device__ CellV identity() { return CellV{0, kLongMax, kLongMin, 0u, kNone, kNone, 0u}; }
    static __host__ __device__ CellV merge(const CellV& a, const CellV& b) {
        CellV r = a;
        r.sum = (long long)((unsigned long long)a.sum + (unsigned long long)b.sum);
        r.count = a.count + b.count;
        // strict tests in arrival order: the smaller window index keeps an equal length
        if (b.min_len < r.min_len || (b.min_len == r.min_len && b.min_pt < r.min_pt)) {
            r.min_len = b.min_len;
            r.min_pt = b.min_pt;
        }
        if (b.max_len > r.max_len || (b.max_len == r.max_len && b.max_pt < r.max_pt)) {
            r.max_len = b.max_len;
            r.max_pt = b.max_pt;
        }
        return r;
    }
};

// a chunk's aggregate for the scan of step 5: the run scan's value since the chunk's last run head
// (flag: it has one) and the chunk's run and cell heads
struct RunPart {
    RunV v;
    unsigned flag, runs, cells, pad;
};
struct RunPartOp {
    __host__ __device__ RunPart operator()(const RunPart& a, const RunPart& b) const {
        RunPart r;
        r.v = b.flag ? b.v : RunV::merge(a.v, b.v);
        r.flag = a.flag | b.flag;
        r.runs = a.runs + b.runs;
        r.cells = a.cells + b.cells;
        r.pad = 0;
        return r;
    }
};
struct CellPartOp {
    __host__ __device__ CellV operator()(const CellV& a, const CellV& b) const {
        if (b.flag) return b;
        CellV r = CellV::merge(a, b);
        r.flag = a.flag;
        return r;
    }
};

template <typename V>
__device__ __forceinline__ V shfl_up_value(const V& v, int d) {
    static_assert(sizeof(V) % 4 == 0, "shuffled by dwords");
    unsigned w[sizeof(V) / 4];
    __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
    for (unsigned k = 0; k < sizeof(V) / 4; k++) w[k] = __shfl_up(w[k], d);
    V r;
    __builtin_memcpy(&r, w, sizeof(V));
    return r;
}

// Inclusive segmented scan over the workgroup's kTB elements in thread order: on return v is the
// merge of the elements from the last head at or before the thread (or the chunk's start) to the
// thread, f whether such a head exists.  sv / sf: kWaves entries of LDS, free again on return.
template <typename V>
__device__ __forceinline__ void block_seg_scan(V& v, unsigned& f, V* sv, unsigned* sf) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const V ov = shfl_up_value(v, d);
        const unsigned of = __shfl_up(f, d);
        if ((int)lane >= d) {
            if (!f) v = V::merge(ov, v);
            f |= of;
        }
    }
    if (lane == 63) {
        sv[wave] = v;
        sf[wave] = f;
    }
    __syncthreads();
    V c = V::identity();
    unsigned cf = 0;
    for (unsigned w = 0; w < wave; w++) {
        if (sf[w]) {
            c = sv[w];
            cf = 1;
        } else {
            c = V::merge(c, sv[w]);
        }
    }
    if (!f) v = V::merge(c, v);
    f |= cf;
    __syncthreads();
}

// Inclusive sum over the workgroup in thread order (values small enough never to carry out).
__device__ __forceinline__ unsigned block_sum_scan(unsigned v, unsigned* sw) {
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(v, d);
        if ((int)lane >= d) v += o;
    }
    if (lane == 63) sw[wave] = v;
    __syncthreads();
    for (unsigned w = 0; w < wave; w++) v += sw[w];
    __syncthreads();
    return v;
}

// ---- 1. cells, checks, rectangle ---------------------------------------------------------------
__global__ void __launch_bounds__(kTB) tagg_locate(const double* x, const double* y, unsigned n, const unsigned* traj_of,
                                                   unsigned T, const unsigned* perm, unsigned n_sel, double mnx, double mny,
                                                   double l, int2* cxy, unsigned* words) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    unsigned err = 0, odd = 0, hx = 0, lx = 0, hy = 0, ly = 0;
    if (j < n_sel) {
        const unsigned p = perm[j];
        int2 c = make_int2(0, 0);
        if (p >= n || traj_of[p] >= T) {
            err = 1;
        } else {
            c.x = d_axis_cell(x[p], mnx, l);
            c.y = d_axis_cell(y[p], mny, l);
            if (c.x < kCellLo || c.x > kCellHi || c.y < kCellLo || c.y > kCellHi) {
                odd = 1;
            } else {
                hx = (unsigned)(c.x - kCellLo);
                lx = (unsigned)(kCellHi - c.x);
                hy = (unsigned)(c.y - kCellLo);
                ly = (unsigned)(kCellHi - c.y);
            }
        }
        cxy[j] = c;
    }
    const unsigned werr = __ballot(err) ? 1u : 0u;
    const unsigned wodd = (unsigned)__popcll(__ballot(odd));
    locate_reduce(werr, wodd, hx, lx, hy, ly, kErrIndex, words);
}

// ---- 2. keys -------------------------------------------------------------------------------------
template <typename K>
__global__ void __launch_bounds__(kTB) tagg_keys(const int2* cxy, unsigned n_sel, int cx0, int cy0, unsigned by, K* key) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    if (j >= n_sel) return;
    const int2 c = cxy[j];
    key[j] = ((K)(unsigned)(c.x - cx0) << by) | (K)(unsigned)(c.y - cy0);
}

// ---- 4. chunk aggregates of the run scan -----------------------------------------------------------
template <typename K>
__global__ void __launch_bounds__(kTB) tagg_partials(const K* key, const unsigned* val, const unsigned* traj_of,
                                                     const long long* ts, unsigned n_sel, unsigned nchunks, long long* ts_s,
                                                     unsigned* tr_s, RunPart* part) {
    __shared__ K sk[kTB + 1];
    __shared__ unsigned st[kTB + 1];
    __shared__ RunV sv[kWaves];
    __shared__ unsigned sf[kWaves];
    const unsigned tid = threadIdx.x, j0 = blockIdx.x * kChunk, j = j0 + tid;
    const bool valid = j < n_sel;
    K k = 0;
    unsigned tr = 0;
    long long t = 0;
    if (valid) {
        k = key[j];
        const unsigned p = val[j];  // < n with traj_of[p] < n_traj: tagg_locate checked perm, the sort permuted it
        tr = traj_of[p];
        t = ts[p];
        ts_s[j] = t;
        tr_s[j] = tr;
    }
    sk[tid + 1] = k;
    st[tid + 1] = tr;
    if (tid == 0 && j0 > 0) {
        sk[0] = key[j0 - 1];
        st[0] = traj_of[val[j0 - 1]];
    }
    __syncthreads();
    const bool ch = valid && (j == 0 || sk[tid] != k);
    const bool rh = valid && (ch || st[tid] != tr);
    RunV v = valid ? RunV{t, t} : RunV::identity();
    unsigned f = rh;
    block_seg_scan(v, f, sv, sf);
    const unsigned runs = (unsigned)__syncthreads_count(rh), cells = (unsigned)__syncthreads_count(ch);
    if (tid == kTB - 1) part[blockIdx.x] = RunPart{v, f, runs, cells, 0u};
    if (tid == 0 && blockIdx.x == 0) part[nchunks] = RunPart{RunV::identity(), 0u, 0u, 0u, 0u};  // carries the totals out
}

// ---- 6. apply ----------------------------------------------------------------------------------------
struct TaggOut {
    int32_t* cell_xy;
    unsigned* cell_count;
    long long* cell_sum;
    long long* cell_avg;
    long long* cell_min;
    unsigned* cell_min_pt;
    long long* cell_max;
    unsigned* cell_max_pt;
    unsigned* visit_off;  // the three visit arrays are null together
    unsigned* visit_traj;
    long long* visit_len;
};

// Math.round(double), JDK 8 (java/lang/Math.java): floor(a + 1/2) computed on the bits, ties
// towards +infinity; beyond 2^52 (and NaN, infinities) the (long) cast, which saturates.
__device__ __forceinline__ long long java_round(double a) {
    const long long bits = __double_as_longlong(a);
    const long long shift = 1074 - ((bits & 0x7ff0000000000000LL) >> 52);
    if ((shift & -64) == 0) {
        long long r = (bits & 0x000fffffffffffffLL) | 0x0010000000000000LL;
        if (bits < 0) r = -r;
        return ((r >> shift) + 1) >> 1;
    }
    if (a != a) return 0;
    if (a >= 9223372036854775807.0) return kLongMax;
    if (a <= -9223372036854775808.0) return kLongMin;
    return (long long)a;
}

__device__ __forceinline__ void emit_cell(const TaggOut& o, unsigned c, const CellV& e) {
    o.cell_count[c] = e.count;
    o.cell_sum[c] = e.sum;
    // TAggregateQuery.java:589: Math.round((sum * 1.0) / (size * 1.0)), emitted only when sum > 0
    o.cell_avg[c] = e.sum > 0 ? java_round((double)e.sum / (double)e.count) : 0;
    o.cell_min[c] = e.min_len;
    o.cell_min_pt[c] = e.min_pt;
    o.cell_max[c] = e.max_len;
    o.cell_max_pt[c] = e.max_pt;
}

template <typename K>
__global__ void __launch_bounds__(kTB) tagg_apply(const K* key, const unsigned* val, const long long* ts_s, const unsigned* tr_s,
                                                  unsigned n_sel, const RunPart* carry, int cx0, int cy0, unsigned by,
                                                  TaggOut out, CellV* part, CellV* open) {
    __shared__ K sk[kTB + 2];
    __shared__ unsigned st[kTB + 2];
    __shared__ RunV sv[kWaves];
    __shared__ CellV sc[kWaves];
    __shared__ unsigned sf[kWaves];
    const unsigned tid = threadIdx.x, j0 = blockIdx.x * kChunk, j = j0 + tid;
    const bool valid = j < n_sel;
    K k = 0;
    unsigned tr = 0, p = 0;
    long long t = 0;
    if (valid) {
        k = key[j];
        p = val[j];
        tr = tr_s[j];
        t = ts_s[j];
    }
    sk[tid + 1] = k;
    st[tid + 1] = tr;
    if (tid == 0 && j0 > 0) {
        sk[0] = key[j0 - 1];
        st[0] = tr_s[j0 - 1];
    }
    if (tid == 1 && j0 + kChunk < n_sel) {
        sk[kTB + 1] = key[j0 + kChunk];
        st[kTB + 1] = tr_s[j0 + kChunk];
    }
    __syncthreads();
    const bool ch = valid && (j == 0 || sk[tid] != k);
    const bool rh = valid && (ch || st[tid] != tr);
    const bool cl = valid && (j + 1 == n_sel || sk[tid + 2] != k);  // the cell's last point
    const bool rl = valid && (cl || st[tid + 2] != tr);             // the run's last point
    const RunPart before = carry[blockIdx.x];

    RunV v = valid ? RunV{t, t} : RunV::identity();
    unsigned f = rh;
    block_seg_scan(v, f, sv, sf);
    if (!f) v = RunV::merge(before.v, v);  // the run began in an earlier chunk
    const long long L = (long long)((unsigned long long)v.mx - (unsigned long long)v.mn);

    const unsigned heads = block_sum_scan((rh ? 1u : 0u) | (ch ? 0x10000u : 0u), sf);
    const unsigned vis = before.runs + (heads & 0xffffu) - 1;  // the point's run (valid points only)
    const unsigned cell = before.cells + (heads >> 16) - 1;    // the point's cell

    CellV e = CellV::identity();
    if (valid) {
        e.count = rh;
        if (rl && !rh) e.sum = L;  // a one-point run has length 0
        if (!rh) {                 // the first point of an objID touches neither extreme
            if (L != kLongMax) {
                e.min_len = L;
                e.min_pt = p;
            }
            if (L != kLongMin) {
                e.max_len = L;
                e.max_pt = p;
            }
        }
    }
    unsigned cf = ch;
    block_seg_scan(e, cf, sc, sf);

    if (rl && out.visit_off) {
        out.visit_traj[vis] = tr;
        out.visit_len[vis] = rh ? 0 : L;
    }
    if (ch) {
        out.cell_xy[2 * (size_t)cell] = cx0 + (int)(unsigned)(k >> by);
        out.cell_xy[2 * (size_t)cell + 1] = cy0 + (int)(unsigned)(k & (((K)1 << by) - 1));
        if (out.visit_off) out.visit_off[cell] = vis;
    }
    if (cl) {
        if (cf) {
            emit_cell(out, cell, e);
        } else {  // began in an earlier chunk: tagg_fix adds what came before
            CellV o = e;
            o.flag = 1;
            open[blockIdx.x] = o;
        }
    }
    if (tid == kTB - 1) {
        e.flag = cf;
        part[blockIdx.x] = e;
    }
}

// ---- 8. the cells that end in a chunk they did not start in -------------------------------------------
__global__ void __launch_bounds__(kTB) tagg_fix(const RunPart* carry, const CellV* cell_carry, const CellV* open,
                                                unsigned nchunks, TaggOut out, unsigned* words) {
    const unsigned c = blockIdx.x * kTB + threadIdx.x;
    if (c > nchunks) return;
    const RunPart before = carry[c];
    if (c == nchunks) {
        if (out.visit_off) out.visit_off[before.cells] = before.runs;
        words[6] = before.cells;
        words[7] = before.runs;
        return;
    }
    const CellV o = open[c];
    if (o.flag && before.cells) emit_cell(out, before.cells - 1, CellV::merge(cell_carry[c], o));
}

// ---- host side -----------------------------------------------------------------------------------------
struct TaggIn {
    const unsigned* traj_of;
    const unsigned* perm;
    const long long* ts;
    unsigned n_sel;
    int cx0, cy0;
    unsigned by, bits;
};

// steps 2-8 for one key width
template <typename K>
int tagg_sorted(geohip_ctx* ctx, const TaggIn& in, const int2* cxy, const TaggOut& out, unsigned* words) {
    hipStream_t st = ctx_stream(ctx);
    const unsigned ns = in.n_sel, nchunks = (ns + kChunk - 1) / kChunk;
    size_t sort_tb = 0, run_tb = 0, cell_tb = 0;
    GEOHIP_CHK(rocprim::radix_sort_pairs(nullptr, sort_tb, (const K*)nullptr, (K*)nullptr, (const unsigned*)nullptr,
                                         (unsigned*)nullptr, ns, 0, in.bits ? in.bits : 1, st));
    GEOHIP_CHK(rocprim::exclusive_scan(nullptr, run_tb, (RunPart*)nullptr, (RunPart*)nullptr, RunPart{}, (size_t)nchunks + 1,
                                       RunPartOp(), st));
    GEOHIP_CHK(rocprim::exclusive_scan(nullptr, cell_tb, (CellV*)nullptr, (CellV*)nullptr, CellV{}, (size_t)nchunks, CellPartOp(), st));
    size_t temp_bytes = sort_tb > run_tb ? sort_tb : run_tb;
    temp_bytes = (temp_bytes > cell_tb ? temp_bytes : cell_tb) + 16;
    K *key, *key2;
    unsigned *val2, *tr_s;
    long long* ts_s;
    void* temp;
    RunPart *rp, *rpx;
    CellV *cp, *cpx, *open;
    int rc = scratch<G_KEY>(ctx, (size_t)ns * sizeof(K), &key);
    if (!rc) rc = scratch<G_KEY2>(ctx, (size_t)ns * sizeof(K), &key2);
    if (!rc) rc = scratch<G_VAL2>(ctx, (size_t)ns * 4, &val2);
    if (!rc) rc = scratch<G_TS>(ctx, (size_t)ns * 8, &ts_s);
    if (!rc) rc = scratch<G_TR>(ctx, (size_t)ns * 4, &tr_s);
    if (!rc) rc = scratch<G_TEMP>(ctx, temp_bytes, &temp);
    // rp | rpx (nchunks + 1 RunPart each, 32 B) | cp | cpx | open (nchunks CellV each, 40 B): 8-byte aligned throughout
    static_assert(sizeof(RunPart) % 8 == 0 && sizeof(CellV) % 8 == 0, "packed back to back");
    char* parts;
    const size_t rp_bytes = ((size_t)nchunks + 1) * sizeof(RunPart), cp_bytes = (size_t)nchunks * sizeof(CellV);
    if (!rc) rc = scratch<G_PARTS>(ctx, 2 * rp_bytes + 3 * cp_bytes, &parts);
    if (rc) return rc;
    rp = reinterpret_cast<RunPart*>(parts);
    rpx = reinterpret_cast<RunPart*>(parts + rp_bytes);
    cp = reinterpret_cast<CellV*>(parts + 2 * rp_bytes);
    cpx = reinterpret_cast<CellV*>(parts + 2 * rp_bytes + cp_bytes);
    open = reinterpret_cast<CellV*>(parts + 2 * rp_bytes + 2 * cp_bytes);
    tlaunch(ctx, tagg_keys<K>, dim3(blocks_for(ns)), dim3(kTB), 0, st, cxy, ns, in.cx0, in.cy0, in.by, key);
    const K* skey = key;
    const unsigned* sval = in.perm;
    if (in.bits) {  // one cell: perm is in (cell, trajectory, index) order as it stands
        size_t tb = temp_bytes;
        GEOHIP_CHK(rocprim::radix_sort_pairs(temp, tb, (const K*)key, key2, in.perm, val2, ns, 0, in.bits, st));
        skey = key2;
        sval = val2;
    }
    tlaunch(ctx, tagg_partials<K>, dim3(nchunks), dim3(kTB), 0, st, skey, sval, in.traj_of, in.ts, ns, nchunks, ts_s, tr_s, rp);
    size_t tb = temp_bytes;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb, rp, rpx, RunPart{RunV::identity(), 0u, 0u, 0u, 0u}, (size_t)nchunks + 1, RunPartOp(), st));
    GEOHIP_CHK(hipMemsetAsync(open, 0, (size_t)nchunks * sizeof(CellV), st));
    tlaunch(ctx, tagg_apply<K>, dim3(nchunks), dim3(kTB), 0, st, skey, sval, (const long long*)ts_s, (const unsigned*)tr_s, ns,
            (const RunPart*)rpx, in.cx0, in.cy0, in.by, out, cp, open);
    tb = temp_bytes;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb, cp, cpx, CellV::identity(), (size_t)nchunks, CellPartOp(), st));
    tlaunch(ctx, tagg_fix, dim3(blocks_for((uint64_t)nchunks + 1)), dim3(kTB), 0, st, (const RunPart*)rpx, (const CellV*)cpx,
            (const CellV*)open, nchunks, out, words);
    GEOHIP_CHK(hipGetLastError());
    return GEOHIP_OK;
}

}  // namespace
}  // namespace geohip

using namespace geohip;

extern "C" {

int geohip_tagg_cells(geohip_ctx* ctx, const geohip_grid* grid, const double* x, const double* y, const int64_t* ts, uint64_t n,
                      const uint32_t* traj_of, const uint32_t* perm, uint64_t n_sel, uint64_t n_traj, int32_t* cell_xy,
                      uint32_t* cell_count, int64_t* cell_sum, int64_t* cell_avg, int64_t* cell_min, uint32_t* cell_min_pt,
                      int64_t* cell_max, uint32_t* cell_max_pt, uint32_t* visit_off, uint32_t* visit_traj, int64_t* visit_len,
                      uint64_t* n_cells, uint64_t* n_visits, uint64_t* n_odd) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!n_cells || !n_visits || !n_odd) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null n_cells / n_visits / n_odd");
    *n_cells = 0;
    *n_visits = 0;
    *n_odd = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tagg_cells takes device memory");
    if (!grid) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null grid");
    if (n > kMaxPoints || n_sel > kMaxPoints || n_traj > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (n_sel > n) return ctx_fail(ctx, GEOHIP_ERR_ARG, "n_sel <= n does not hold");
    const bool visits = visit_off || visit_traj || visit_len;
    if (visits && !(visit_off && visit_traj && visit_len))
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "visit_off, visit_traj and visit_len are null together");
    hipStream_t st = ctx_stream(ctx);
    if (n_sel == 0) {
        if (visits) GEOHIP_CHK(hipMemsetAsync(visit_off, 0, 4, st));
        return GEOHIP_OK;
    }
    if (!x || !y || !ts || !traj_of || !perm || !cell_xy || !cell_count || !cell_sum || !cell_avg || !cell_min ||
        !cell_min_pt || !cell_max || !cell_max_pt)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    const unsigned ns = (unsigned)n_sel;
    int2* cxy;
    unsigned* words;
    rc = scratch<G_CXY>(ctx, (size_t)ns * sizeof(int2), &cxy);
    if (!rc) rc = scratch<G_WORDS>(ctx, 64, &words);
    if (rc) return rc;
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    tlaunch(ctx, tagg_locate, dim3(blocks_for(ns)), dim3(kTB), 0, st, x, y, (unsigned)n, traj_of, (unsigned)n_traj, perm, ns,
            grid->min_x, grid->min_y, grid->cell_len, cxy, words);
    WordsHead head;  // the error bits, the points outside [kCellLo, kCellHi], the rectangle as four maxima
    rc = read_words_head(ctx, words, st, &head);
    if (rc) return rc;
    const unsigned odd = head.count;
    if (head.err & kErrIndex) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tagg_cells: perm entry >= n, or traj_of[perm[j]] >= n_traj");
    if (odd) {
        *n_odd = odd;
        return ctx_fail(ctx, GEOHIP_ERR_ARG,
                        "a point's cell index leaves [-9999, 99999]: its \"%05d%05d\" key does not split uniquely; *n_odd = such points");
    }
    TaggIn in;
    in.traj_of = traj_of;
    in.perm = perm;
    in.ts = reinterpret_cast<const long long*>(ts);
    in.n_sel = ns;
    const int cx1 = kCellLo + (int)head.hx, cy1 = kCellLo + (int)head.hy;
    in.cx0 = kCellHi - (int)head.lx;
    in.cy0 = kCellHi - (int)head.ly;
    const unsigned bx = bits_for((unsigned)(cx1 - in.cx0 + 1));
    in.by = bits_for((unsigned)(cy1 - in.cy0 + 1));
    in.bits = bx + in.by;
    TaggOut out;
    out.cell_xy = cell_xy;
    out.cell_count = cell_count;
    out.cell_sum = reinterpret_cast<long long*>(cell_sum);
    out.cell_avg = reinterpret_cast<long long*>(cell_avg);
    out.cell_min = reinterpret_cast<long long*>(cell_min);
    out.cell_min_pt = cell_min_pt;
    out.cell_max = reinterpret_cast<long long*>(cell_max);
    out.cell_max_pt = cell_max_pt;
    out.visit_off = visit_off;
    out.visit_traj = visit_traj;
    out.visit_len = reinterpret_cast<long long*>(visit_len);
    rc = in.bits <= 32 ? tagg_sorted<uint32_t>(ctx, in, cxy, out, words) : tagg_sorted<uint64_t>(ctx, in, cxy, out, words);
    if (rc) return rc;
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipMemcpyAsync(pin, words + 6, 8, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    *n_cells = pin[0] & 0xffffffffu;
    *n_visits = pin[0] >> 32;
    return GEOHIP_OK;
}

}  // extern "C"
