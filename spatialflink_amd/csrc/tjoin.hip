// tjoin.hip -- the trajectory join PointPointTJoinQuery (window form) on the device: geohip_tjoin_pp.
//
// Reference (paths relative to the reference's src/main/java/GeoFlink):
//   window form   spatialOperators/tJoin/PointPointTJoinQuery.java:183-338: both streams keyed by
//                 objID into windowed trajectories (TJoinQuery.java:158-192, more than one point),
//                 the query points replicated into uGrid.getNeighboringCells(joinDistance, q)
//                 (TJoinQuery.java:195-211, UniformGrid.java:261-293), joined with the ordinary points
//                 on the cell key under DistanceFunctions.getPointPointEuclideanDistance <= joinDistance
//                 (:213-240), reduced per ordinary objID to a map query objID -> point (:246-288) and
//                 joined back to the trajectories of both sides (:293-337);
//   predicate     utils/DistanceFunctions.java:60-63: sqrt(dy*dy + dx*dx), NOT JTS point.distance
//                 (Math.hypot), which geohip_join_pp restates: the two differ by an ulp in about one
//                 pair of eight, so this call decides its own pairs.
//
// The two closing joins keep only the objIDs of each (ordinary point, query point) hit, so the
// window's result is a set: (a, b) for every pair of trajectories with some joining point pair.
//
// Kernels (kTB = 256 threads; no workgroup waits for another):
//   1. tj_locate   per ordinary point: its trajectory (checked), its cell (d_axis_cell); counts the
//                  points that take part (selected, trajectory of >= min_points points, cell inside the
//                  grid) and their cell rectangle (one set of atomics per workgroup);
//   2. tj_qrect    per query point its cell square clipped to the grid, with the reference's error
//                  cases (d_neighbor_square, locate.h: the one jq_rect of cell_kernels.hip calls);
//      -- read-back: errors, the count, the rectangle --
//   3. tj_keys     key = (cx - cx0) * H + (cy - cy0) inside the rectangle, W * H for a point that
//                  takes no part; rocPRIM stable LSD radix sort of (key, index) over bits(W * H + 1);
//   4. tj_records  the sorted stream of 24-byte (x, y, trajectory) records: the probe gathers nothing;
//   5. tj_cells    cell starts over the rectangle (a lower bound per cell) while W * H + 1 fits the
//                  budget; beyond it the probe finds a span's ends by the same search;
//   6. tj_qwidth   each query rectangle clipped to the occupied rectangle and its column count;
//                  rocPRIM exclusive scan -> the (query point, column) work items;
//   7. tj_probe    a wave per item strides its span (one column of a rectangle is one contiguous run
//                  of the sorted stream) 64 records a step: the exact predicate behind a squared
//                  screen, hits deduplicated among the lanes through LDS, then the u64 key
//                  ta << bits(ntb) | tb into an open-addressing hash set: a load per probe and a 64-bit
//                  CAS only at an empty slot.  A slot only ever goes from empty to one key, so a stale
//                  read costs one more CAS and never a wrong answer;
//      -- read-back: the distinct count; above half load the table grows x4 and 7 runs again --
//   8. rocPRIM select of the occupied slots, radix sort over bits(nta) + bits(ntb), tj_write.
// The result is a set filled by idempotent inserts and then sorted: it does not depend on
// execution order.  Extra memory: O(na) keys and records, O(W * H) cell starts within the budget,
// O(nb) rectangles, O(distinct pairs) slots (or 2 nta ntb where that is small).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include "geohip.h"
#include "traj_common.h"

namespace geohip {
namespace {

constexpr unsigned long long kEmpty = ~0ull;  // no key: ta < 2^30, so a key's top bit is clear
// cell starts are built while the occupied rectangle holds fewer cells (64 MiB of offsets)
constexpr uint64_t kTJoinCellBudget = 1ull << 24;
// hash set: sized once at the power of two >= 2 nta ntb while that is within kTableOnce slots
// (256 MiB); otherwise kTableFirst slots, x4 after every pass that ends above half load
constexpr uint64_t kTableOnce = 1ull << 25;
constexpr uint64_t kTableFirst = 1ull << 22;
constexpr uint64_t kTableMax = 1ull << 30;
constexpr unsigned kMaxProbe = 1u << 14;  // a probe chain this long abandons the pass (the table grows)

// scratch slots (kCallSlots, traj_common.h)
enum TSlot { T_WORDS, T_KEY, T_KEY2, T_REC, T_CELL, T_RECT, T_TEMP, T_TABLE, T_OUT };

// words block (16 u32): [0] error bits, [1] ordinary points that take part, [2..5] their cell
// rectangle as maxima of cx, n - 1 - cx, cy, n - 1 - cy, [6] keys inserted by the probe pass,
// [7] the pass gave up on a probe chain, [8] slots selected
constexpr unsigned kErrTrajA = 1u;   // traj_of_a entry >= nta
constexpr unsigned kErrTrajB = 2u;   // traj_of_b entry >= ntb
constexpr unsigned kErrKey = 4u;     // query key: NumberFormatException
constexpr unsigned kErrLoop = 8u;    // query square: a loop that never ends
constexpr unsigned kWordsBytes = 64;

struct TjRec {
    double x, y;
    unsigned traj, pad;
};
static_assert(sizeof(TjRec) == 24, "24-byte records");

struct TjGeom {
    double mnx, mny, l;
    int32_t n, lc;   // cells per side, candidate layers
    int all_cells;   // r == 0: every cell (UniformGrid.java:264-266)
    unsigned min_points;
};

// Whether ordinary point i takes part, and its cell: selected, its trajectory a trajectory under
// min_points, its unclipped cell a cell of the grid (the key of any other cell equals no
// replica's: it is longer than 10 characters or carries a '-').  err: traj_of[i] >= nt.
__device__ __forceinline__ bool a_point(const double* x, const double* y, const unsigned* traj_of, const unsigned* traj_off,
                                        unsigned nt, unsigned i, const TjGeom& g, int32_t& cx, int32_t& cy, bool& err) {
    const unsigned t = traj_of[i];
    err = false;
    if (t == kNone) return false;
    if (t >= nt) {
        err = true;
        return false;
    }
    if (traj_off[t + 1] - traj_off[t] < g.min_points) return false;
    cx = d_axis_cell(x[i], g.mnx, g.l);
    cy = d_axis_cell(y[i], g.mny, g.l);
    return cx >= 0 && cx < g.n && cy >= 0 && cy < g.n;
}

// ---- 1. ordinary points: checks, count, rectangle ---------------------------------------------
__global__ void __launch_bounds__(kTB) tj_locate(const double* x, const double* y, unsigned n, const unsigned* traj_of,
                                                 const unsigned* traj_off, unsigned nt, TjGeom g, unsigned* words) {
    unsigned hx = 0, lx = 0, hy = 0, ly = 0, cnt = 0;
    bool err = false;
    // a grid-stride loop: the atomics below all go to one line, so their number is the grid's, not n / 256
    for (unsigned i = blockIdx.x * kTB + threadIdx.x; i < n; i += gridDim.x * kTB) {
        int32_t cx = 0, cy = 0;
        bool e;
        if (a_point(x, y, traj_of, traj_off, nt, i, g, cx, cy, e)) {
            cnt++;
            hx = max(hx, (unsigned)cx);
            lx = max(lx, (unsigned)(g.n - 1 - cx));
            hy = max(hy, (unsigned)cy);
            ly = max(ly, (unsigned)(g.n - 1 - cy));
        }
        err = err || e;
    }
    const unsigned werr = __ballot(err) ? 1u : 0u;
    locate_reduce(werr, wave_sum(cnt), hx, lx, hy, ly, kErrTrajA, words);
}

// ---- 2. query squares ------------------------------------------------------------------------------
// UniformGrid.getNeighboringCells (UniformGrid.java:261-293) of every selected query point
// (d_neighbor_square, locate.h).  The reference replicates a point before it knows the point's
// trajectory, so the error cases count for one-point trajectories too; an unselected point takes no
// part at all.
__global__ void __launch_bounds__(kTB) tj_qrect(const double* qx, const double* qy, unsigned nq, const unsigned* traj_of,
                                                const unsigned* traj_off, unsigned nt, TjGeom g, QRect* rect, unsigned* words) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= nq) return;
    const QRect none{1, 0, 1, 0};
    const unsigned t = traj_of[i];
    if (t == kNone) {
        rect[i] = none;
        return;
    }
    if (t >= nt) {
        atomicOr(&words[0], kErrTrajB);
        rect[i] = none;
        return;
    }
    QRect R{0, g.n - 1, 0, g.n - 1};
    if (!g.all_cells) {
        const int st = d_neighbor_square(d_axis_cell(qx[i], g.mnx, g.l), d_axis_cell(qy[i], g.mny, g.l), g.lc, g.n, R);
        if (st) atomicOr(&words[0], st == 1 ? kErrKey : kErrLoop);
    }
    if (traj_off[t + 1] - traj_off[t] < g.min_points) R = none;  // no trajectory: its hits are dropped
    rect[i] = R;
}

// ---- 3. keys ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTB) tj_keys(const double* x, const double* y, unsigned n, const unsigned* traj_of,
                                               const unsigned* traj_off, unsigned nt, TjGeom g, int cx0, int cy0, unsigned H,
                                               unsigned none_key, unsigned* key, unsigned* val) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    int32_t cx = 0, cy = 0;
    bool err;
    const bool in = a_point(x, y, traj_of, traj_off, nt, i, g, cx, cy, err);
    key[i] = in ? (unsigned)(cx - cx0) * H + (unsigned)(cy - cy0) : none_key;
    val[i] = i;
}

// ---- 4. records ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTB) tj_records(const unsigned* sval, unsigned nv, const double* x, const double* y,
                                                  const unsigned* traj_of, TjRec* rec) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    if (j >= nv) return;
    const unsigned i = sval[j];  // a point that takes part: tj_keys gave every other the last key
    rec[j] = TjRec{x[i], y[i], traj_of[i], 0u};
}

// ---- 5. cell starts ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTB) tj_cells(const unsigned* skey, unsigned nv, unsigned ncells, unsigned* cell_off) {
    const unsigned c = blockIdx.x * kTB + threadIdx.x;
    if (c > ncells) return;
    cell_off[c] = lower_bound(skey, nv, c);
}

// ---- 6. query rectangles inside the occupied rectangle ------------------------------------------------
__global__ void __launch_bounds__(kTB) tj_qwidth(QRect* rect, unsigned nq, int cx0, int cx1, int cy0, int cy1,
                                                 unsigned long long* width) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i > nq) return;
    unsigned long long w = 0;
    if (i < nq) {
        QRect R = rect[i];
        if (R.x0 <= R.x1 && R.y0 <= R.y1) {
            R.x0 = R.x0 > cx0 ? R.x0 : cx0;
            R.x1 = R.x1 < cx1 ? R.x1 : cx1;
            R.y0 = R.y0 > cy0 ? R.y0 : cy0;
            R.y1 = R.y1 < cy1 ? R.y1 : cy1;
            if (R.x0 <= R.x1 && R.y0 <= R.y1) w = (unsigned long long)(R.x1 - R.x0 + 1);
            rect[i] = R;
        }
    }
    width[i] = w;  // entry nq = 0: the scan carries the total there
}

// ---- 7. probe ----------------------------------------------------------------------------------------
struct TjProbe {
    const TjRec* rec;
    const unsigned* skey;
    const unsigned* cell_off;  // null: spans by search in skey
    unsigned nv;
    unsigned nq;
    const double* qx;
    const double* qy;
    const unsigned* traj_of_q;
    const QRect* rect;
    const unsigned long long* item_off;  // nq + 1
    int cx0, cy0;
    unsigned H;
    unsigned kb;  // key = ta << kb | tb
    double r, r2lo, r2hi;
    unsigned long long* table;
    unsigned long long hash_mask;
    unsigned slot_mask;  // slots - 1
    unsigned* words;
};

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {  // splitmix64's finalizer
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(kTB) tj_probe(TjProbe a) {
    __shared__ unsigned owner[kWaves][64];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long nw = (unsigned long long)gridDim.x * kWaves;
    const unsigned long long total = a.item_off[a.nq];
    const unsigned half = (a.slot_mask >> 1) + 1;
    const unsigned chain = a.slot_mask < kMaxProbe ? a.slot_mask : kMaxProbe;
    for (unsigned long long it = (unsigned long long)blockIdx.x * kWaves + wave; it < total; it += nw) {
        // a pass that is over half load, or gave up, is run again with a larger table: stop early
        const int stop = __hip_atomic_load(&a.words[7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                         __hip_atomic_load(&a.words[6], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > half;
        if (__builtin_amdgcn_readfirstlane(stop)) break;  // one answer for the wave
        // the item's query point: the last q with item_off[q] <= it (its width is not 0)
        unsigned lo = 0, hi = a.nq;
        while (hi - lo > 1) {
            const unsigned mid = lo + (hi - lo) / 2;
            if (a.item_off[mid] <= it) lo = mid;
            else hi = mid;
        }
        const unsigned q = lo;
        const QRect R = a.rect[q];
        const unsigned col = (unsigned)(R.x0 - a.cx0) + (unsigned)(it - a.item_off[q]);
        const unsigned k0 = col * a.H + (unsigned)(R.y0 - a.cy0), k1 = col * a.H + (unsigned)(R.y1 - a.cy0);
        unsigned beg, end;
        if (a.cell_off) {
            beg = a.cell_off[k0];
            end = a.cell_off[k1 + 1];
        } else {
            beg = lower_bound(a.skey, a.nv, k0);
            end = lower_bound(a.skey, a.nv, k1 + 1);
        }
        const double qx = a.qx[q], qy = a.qy[q];
        const unsigned long long tb = a.traj_of_q[q];
        unsigned added = 0;
        for (unsigned base = beg; base < end; base += 64) {
            const unsigned j = base + lane;
            bool hit = false;
            unsigned ta = 0;
            if (j < end) {
                const TjRec p = a.rec[j];
                ta = p.traj;
                // DistanceFunctions.java:60-63 with (lon, lat) = p and (lon1, lat1) = q
                const double dy = qy - p.y, dx = qx - p.x;
                const double d2 = dy * dy + dx * dx;
                // screen (pp_screen_bounds): d2 is the very operand of the square root, so below
                // r2lo = r^2 (1 - 2^-40) the rounded root is below r and above r2hi it is above;
                // NaN fails both compares and takes the exact path, where it fails too
                if (d2 < a.r2lo) hit = true;
                else if (d2 > a.r2hi) hit = false;
                else hit = __builtin_sqrt(d2) <= a.r;
            }
            if (__ballot(hit) == 0) continue;
            // among the lanes that hit the same trajectory one inserts: each writes its lane at
            // owner[ta mod 64], reads the slot's survivor and yields to it when that lane holds the
            // same ta (two trajectories sharing a slot both insert: nothing is lost)
            if (hit) owner[wave][ta & 63u] = lane;
            wave_lds_sync();
            const unsigned own = hit ? owner[wave][ta & 63u] : lane;
            wave_lds_sync();
            const unsigned own_ta = __shfl(ta, (int)own);
            bool ins = hit && (own == lane || own_ta != ta);
            bool fresh = false, gave_up = false;
            if (ins) {
                const unsigned long long key = ((unsigned long long)ta << a.kb) | tb;
                unsigned s = (unsigned)(mix64(key) & a.hash_mask) & a.slot_mask;
                for (unsigned probes = 0;; probes++) {
                    unsigned long long cur = __hip_atomic_load(&a.table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (cur == kEmpty) {
                        cur = atomicCAS(&a.table[s], kEmpty, key);
                        if (cur == kEmpty) {
                            fresh = true;
                            break;
                        }
                    }
                    if (cur == key) break;
                    if (probes >= chain) {
                        gave_up = true;
                        break;
                    }
                    s = (s + 1) & a.slot_mask;
                }
            }
            added += (unsigned)__popcll(__ballot(fresh));
            if (__ballot(gave_up) && lane == 0) atomicOr(&a.words[7], 1u);
        }
        if (added && lane == 0) atomicAdd(&a.words[6], added);
    }
}

// ---- 8. emit ---------------------------------------------------------------------------------------------
struct IsKey {
    __host__ __device__ bool operator()(const unsigned long long& k) const { return k != kEmpty; }
};

__global__ void __launch_bounds__(kTB) tj_write(const unsigned long long* key, unsigned m, unsigned kb, unsigned* out) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= m) return;
    const unsigned long long k = key[i];
    out[2 * (size_t)i] = (unsigned)(k >> kb);
    out[2 * (size_t)i + 1] = (unsigned)(k & ((1ull << kb) - 1));
}

}  // namespace
}  // namespace geohip

using namespace geohip;

extern "C" {

int geohip_tjoin_pp(geohip_ctx* ctx, const geohip_grid* grid, const double* ax, const double* ay, uint64_t na,
                    const uint32_t* traj_of_a, const uint32_t* traj_off_a, uint64_t nta, const double* bx, const double* by,
                    uint64_t nb, const uint32_t* traj_of_b, const uint32_t* traj_off_b, uint64_t ntb, double r,
                    uint32_t min_points, uint32_t* out_tpairs, uint64_t cap, uint64_t* out_count) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!out_count) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out_count");
    *out_count = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tjoin_pp takes device memory");
    rc = check_grid_basic(ctx, grid, "grid");
    if (rc) return rc;
    if (na > kMaxPoints || nb > kMaxPoints || nta > kMaxPoints || ntb > kMaxPoints)
        return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (cap && !out_tpairs) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out_tpairs");
    if ((na && (!ax || !ay || !traj_of_a)) || (nb && (!bx || !by || !traj_of_b)) || (nta && !traj_off_a) || (ntb && !traj_off_b))
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    const bool all_cells = (r == 0);  // UniformGrid.java:264-266
    const int32_t lc = layers_candidate(*grid, r);
    if (!all_cells && lc <= 0)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "candidateNeighboringLayers cannot be 0 or less (UniformGrid.java:272-276)");
    if (nb == 0) return GEOHIP_OK;  // nothing is replicated: no pair and no error
    hipStream_t st = ctx_stream(ctx);
    const uint64_t* dbg = ctx_tjoin_debug(ctx);
    const TjGeom g{grid->min_x, grid->min_y, grid->cell_len, grid->n, lc, all_cells ? 1 : 0, min_points};
    const unsigned una = (unsigned)na, unb = (unsigned)nb;

    unsigned* words;
    QRect* rect;
    // rect (nb QRect, 16 B each) | width (nb + 1 u64) | item_off (nb + 1 u64)
    char* qblock;
    const size_t rect_bytes = (size_t)unb * sizeof(QRect), off_bytes = ((size_t)unb + 1) * 8;
    rc = scratch<T_WORDS>(ctx, kWordsBytes, &words);
    if (!rc) rc = scratch<T_RECT>(ctx, rect_bytes + 2 * off_bytes, &qblock);
    if (rc) return rc;
    rect = reinterpret_cast<QRect*>(qblock);
    unsigned long long* width = reinterpret_cast<unsigned long long*>(qblock + rect_bytes);
    unsigned long long* item_off = reinterpret_cast<unsigned long long*>(qblock + rect_bytes + off_bytes);
    GEOHIP_CHK(hipMemsetAsync(words, 0, kWordsBytes, st));
    if (na) {
        const unsigned want = blocks_for(una), most = (unsigned)ctx_cus(ctx) * 8u;
        tlaunch(ctx, tj_locate, dim3(want < most ? want : most), dim3(kTB), 0, st, ax, ay, una, traj_of_a, traj_off_a,
                (unsigned)nta, g, words);
    }
    tlaunch(ctx, tj_qrect, dim3(blocks_for(unb)), dim3(kTB), 0, st, bx, by, unb, traj_of_b, traj_off_b, (unsigned)ntb, g, rect, words);
    WordsHead head;  // the error bits, the points that take part, their rectangle as four maxima
    rc = read_words_head(ctx, words, st, &head);
    if (rc) return rc;
    const unsigned err = head.err, nv = head.count;
    if (err & kErrTrajA) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tjoin_pp: traj_of_a entry >= nta");
    if (err & kErrTrajB) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_tjoin_pp: traj_of_b entry >= ntb");
    if (err & kErrKey)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "query point cell key does not parse (NumberFormatException, HelperClass.java:263-276)");
    if (err & kErrLoop)
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "query point neighbourhood reaches Integer.MAX_VALUE: the reference loop does not terminate");
    if (nv == 0) return GEOHIP_OK;
    const int cx1 = (int)head.hx, cx0 = grid->n - 1 - (int)head.lx;
    const int cy1 = (int)head.hy, cy0 = grid->n - 1 - (int)head.ly;
    const uint64_t W = (uint64_t)(cx1 - cx0 + 1), H = (uint64_t)(cy1 - cy0 + 1), ncells = W * H;
    if (ncells >= 0xffffffffull)
        return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "the occupied cell rectangle holds 2^32 - 1 cells or more");
    const unsigned key_bits = bits_for(ncells + 1);  // keys 0 .. ncells
    const uint64_t cell_budget = dbg[2] ? dbg[2] : kTJoinCellBudget;
    const bool csr = ncells + 1 <= cell_budget;

    // 3-5: bin the ordinary window
    unsigned *key, *key2, *cell_off = nullptr;
    TjRec* rec;
    void* temp;
    size_t sort_tb = 0, scan_tb = 0;
    GEOHIP_CHK(rocprim::radix_sort_pairs(nullptr, sort_tb, (const unsigned*)nullptr, (unsigned*)nullptr, (const unsigned*)nullptr,
                                         (unsigned*)nullptr, una, 0, key_bits, st));
    GEOHIP_CHK(rocprim::exclusive_scan(nullptr, scan_tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, 0ull,
                                       (size_t)unb + 1, rocprim::plus<unsigned long long>(), st));
    size_t temp_bytes = (sort_tb > scan_tb ? sort_tb : scan_tb) + 16;
    rc = scratch<T_KEY>(ctx, (size_t)una * 8, &key);  // key | val
    if (!rc) rc = scratch<T_KEY2>(ctx, (size_t)una * 8, &key2);
    if (!rc) rc = scratch<T_REC>(ctx, (size_t)nv * sizeof(TjRec), &rec);
    if (!rc) rc = scratch<T_TEMP>(ctx, temp_bytes, &temp);
    if (!rc && csr) rc = scratch<T_CELL>(ctx, (size_t)(ncells + 1) * 4, &cell_off);
    if (rc) return rc;
    unsigned *val = key + una, *val2 = key2 + una;
    tlaunch(ctx, tj_keys, dim3(blocks_for(una)), dim3(kTB), 0, st, ax, ay, una, traj_of_a, traj_off_a, (unsigned)nta, g, cx0, cy0,
            (unsigned)H, (unsigned)ncells, key, val);
    size_t tb = temp_bytes;
    GEOHIP_CHK(rocprim::radix_sort_pairs(temp, tb, (const unsigned*)key, key2, (const unsigned*)val, val2, una, 0, key_bits, st));
    tlaunch(ctx, tj_records, dim3(blocks_for(nv)), dim3(kTB), 0, st, (const unsigned*)val2, nv, ax, ay, traj_of_a, rec);
    if (csr)
        tlaunch(ctx, tj_cells, dim3(blocks_for(ncells + 1)), dim3(kTB), 0, st, (const unsigned*)key2, nv, (unsigned)ncells, cell_off);
    // 6: the work items
    tlaunch(ctx, tj_qwidth, dim3(blocks_for((uint64_t)unb + 1)), dim3(kTB), 0, st, rect, unb, cx0, cx1, cy0, cy1, width);
    tb = temp_bytes;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb, width, item_off, 0ull, (size_t)unb + 1, rocprim::plus<unsigned long long>(), st));
    GEOHIP_CHK(hipGetLastError());

    // 7: probe into the hash set, growing it until a pass ends at or below half load
    const unsigned kb = bits_for(ntb), ka = bits_for(nta);
    double r2lo, r2hi;
    pp_screen_bounds(r, &r2lo, &r2hi);
    const uint64_t all_pairs = nta * ntb;  // <= 2^60
    uint64_t slots;
    if (dbg[0]) slots = pow2_at_least(dbg[0]);
    else if (2 * all_pairs <= kTableOnce) slots = pow2_at_least(2 * all_pairs);
    else slots = kTableFirst;
    static const int resident = [] {
        int nbk = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nbk, tj_probe, kTB, 0) == hipSuccess && nbk > 0 ? nbk : 4;
    }();
    const unsigned probe_blocks = (unsigned)ctx_cus(ctx) * (unsigned)(resident < 8 ? resident : 8);
    uint64_t count = 0;
    unsigned long long* table = nullptr;
    uint64_t* pin = ctx_pinned(ctx);
    for (;;) {
        if (slots > kTableMax) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^29 distinct trajectory pairs");
        rc = scratch<T_TABLE>(ctx, (size_t)slots * 8, &table);
        if (rc) return rc;
        GEOHIP_CHK(hipMemsetAsync(table, 0xff, (size_t)slots * 8, st));
        GEOHIP_CHK(hipMemsetAsync(words + 6, 0, 8, st));
        TjProbe p;
        p.rec = rec;
        p.skey = key2;
        p.cell_off = cell_off;
        p.nv = nv;
        p.nq = unb;
        p.qx = bx;
        p.qy = by;
        p.traj_of_q = traj_of_b;
        p.rect = rect;
        p.item_off = item_off;
        p.cx0 = cx0;
        p.cy0 = cy0;
        p.H = (unsigned)H;
        p.kb = kb;
        p.r = r;
        p.r2lo = r2lo;
        p.r2hi = r2hi;
        p.table = table;
        p.hash_mask = dbg[1];
        p.slot_mask = (unsigned)(slots - 1);
        p.words = words;
        tlaunch(ctx, tj_probe, dim3(probe_blocks), dim3(kTB), 0, st, p);
        GEOHIP_CHK(hipGetLastError());
        GEOHIP_CHK(hipMemcpyAsync(pin, words + 6, 8, hipMemcpyDeviceToHost, st));
        GEOHIP_CHK(hipStreamSynchronize(st));
        ctx_tjoin_debug(ctx)[3]++;  // probe passes (scripts/tjoin_time.py reads it through the hook)
        count = pin[0] & 0xffffffffu;
        const bool gave_up = (pin[0] >> 32) != 0;
        if (!gave_up && count <= slots / 2) break;
        slots *= 4;
    }
    *out_count = count;
    if (count > cap) return ctx_fail(ctx, GEOHIP_ERR_CAPACITY, "output capacity too small; *out_count = required");
    if (count == 0) return GEOHIP_OK;

    // 8: the occupied slots, ascending by (ta, tb)
    const unsigned m = (unsigned)count;
    unsigned long long* okey;
    size_t sel_tb = 0, ksort_tb = 0;
    GEOHIP_CHK(rocprim::select(nullptr, sel_tb, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (unsigned*)nullptr,
                               (size_t)slots, IsKey(), st));
    GEOHIP_CHK(rocprim::radix_sort_keys(nullptr, ksort_tb, (const unsigned long long*)nullptr, (unsigned long long*)nullptr, m, 0,
                                        ka + kb ? ka + kb : 1, st));
    temp_bytes = (sel_tb > ksort_tb ? sel_tb : ksort_tb) + 16;
    rc = scratch<T_OUT>(ctx, (size_t)m * 16, &okey);
    if (!rc) rc = scratch<T_TEMP>(ctx, temp_bytes, &temp);
    if (rc) return rc;
    tb = temp_bytes;
    GEOHIP_CHK(rocprim::select(temp, tb, table, okey, words + 8, (size_t)slots, IsKey(), st));
    const unsigned long long* sorted = okey;
    if (ka + kb) {
        tb = temp_bytes;
        GEOHIP_CHK(rocprim::radix_sort_keys(temp, tb, (const unsigned long long*)okey, okey + m, m, 0, ka + kb, st));
        sorted = okey + m;
    }
    tlaunch(ctx, tj_write, dim3(blocks_for(m)), dim3(kTB), 0, st, sorted, m, kb, out_tpairs);
    GEOHIP_CHK(hipGetLastError());
    return GEOHIP_OK;
}

// Test hook: table_slots != 0 forces the hash set's first size (rounded up to a power of two, at
// least 2) in place of the sizing policy; every hash is ANDed with hash_mask (0: one probe chain
// for all keys, which holds at most 2^14 of them).  geohip_debug_tjoin(ctx, 0, ~0) restores the
// defaults.
int geohip_debug_tjoin(geohip_ctx* ctx, uint64_t table_slots, uint64_t hash_mask) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    uint64_t* d = ctx_tjoin_debug(ctx);
    d[0] = table_slots;
    d[1] = hash_mask;
    return GEOHIP_OK;
}

// Test hook: the cell budget of the cell starts (0: kTJoinCellBudget).  With a budget below the
// occupied rectangle's cell count + 1 the probe finds its spans by search in the sorted keys.
int geohip_debug_tjoin_cell_budget(geohip_ctx* ctx, uint64_t cells) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    ctx_tjoin_debug(ctx)[2] = cells;
    return GEOHIP_OK;
}

// Test hook: the probe passes this ctx has run since its creation.
int geohip_debug_tjoin_passes(geohip_ctx* ctx, uint64_t* out) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!out) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out");
    *out = ctx_tjoin_debug(ctx)[3];
    return GEOHIP_OK;
}

}  // extern "C"
