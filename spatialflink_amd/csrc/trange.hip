// trange.hip -- the trajectory range query PointPolygonTRangeQuery on the device: a per-point
// class against a polygon set (geohip_trange_classify) and the filter that keeps the trajectories
// owning a hit point (geohip_traj_filter_hit).
//
// Reference (paths relative to the reference's src/main/java/GeoFlink):
//   cell filter  spatialOperators/tRange/PointPolygonTRangeQuery.java:55-59, 92-97 (polygonsGridCellIDs =
//                the union of the polygons' gridIDsSet, utils/HelperClass.java:123-143, unclipped) and
//                :62-71, 100-109 (a point passes iff its own gridID, HelperClass.java:104-120, is in it);
//   containment  :81, :130: poly.polygon.contains(p.point.getEnvelope()) -- JTS Geometry.contains: the
//                polygon's envelope covers the point (a NaN coordinate fails) and the point's location
//                (PointLocator.locateInPolygon) is INTERIOR: shell EXTERIOR or BOUNDARY -> no; a hole
//                whose envelope includes the point with the point on or inside it -> no;
//   window form  :90-177: a trajectory (objID) with one contained point is emitted with all its points.
//
// geohip_trange_classify, one streaming pass over x / y (trange_classify):
//   per point its cell (d_axis_cell, the expression every kernel uses), then the cell's polygon
//   list: the host plan's cell -> polygon CSR over the bounding rectangle of the polygons'
//   rectangles (two loads; a cell no polygon covers costs the same whatever npoly), or, when that
//   rectangle is beyond the budget (kTRangeCellBudget), a scan of the rectangle list.  A point
//   outside the set gets class 0 at once; the others are queued per wave in LDS (as CandQueue
//   does for the range query; a wave takes runs of kWaveBatches consecutive 64-point batches, so
//   the queue fills across them) and located 64 at a time, one point per lane, each lane walking its
//   cell's polygons in ascending order until one contains it.  A polygon whose crossing list for
//   the point is longer than kLaneSegs segments is not walked by its lane: the wave takes these
//   (point, polygon) pairs one by one, 64 segments a step, and reduces the per-ring masks.
//   The locator is the range query's (count_segment, per-ring boundary / parity masks over chunks
//   of 64 rings, y-slab crossing lists), read tri-state: INTERIOR only.  No distance is computed.
//   Class-2 indices: rocPRIM select over the class bytes (ascending), after the count is known.
// geohip_traj_filter_hit: mark (plain stores of 1) the trajectories of the points at or above the
//   threshold, exclusive scans of the marks and of the marked trajectories' lengths (rocPRIM),
//   then per selected point a copy into its trajectory's new slice.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "geohip.h"
#include "traj_common.h"
#include "trange.h"

namespace geohip {
namespace {

constexpr int kQueue = 128;          // per-wave queue of points whose cell is in the set
constexpr unsigned kLaneSegs = 48;   // longer crossing lists are walked by the whole wave
constexpr unsigned kWaveBatches = 8;  // consecutive 64-point batches a wave takes at a time

// scratch slots (kCallSlots, traj_common.h)
enum RSlot { R_FLAG, R_NEWID, R_LEN, R_NEWOFF, R_TEMP = 6, R_WORDS = 7 };

// words block: [0] error bits, [1] class-2 points
constexpr unsigned kErrIndex = 1u;  // malformed group: see geohip_traj_filter_hit

struct TRPoly {
    double bb[4];         // the shell's envelope: minx, miny, maxx, maxy
    double sy0, sinv;     // slab of y (slab_of)
    uint32_t voff, nv;    // closed rings back to back in vx / vy
    uint32_t nring, eoff; // ring envelopes at env[4 * eoff ...]
    uint32_t ns, loff;    // y slabs (0: every segment is visited) and their block in the u16 blob
};

struct TRArgs {
    const double* x;
    const double* y;
    uint64_t n;
    double mnx, mny, l;
    const TRPoly* polys;
    const double* vx;
    const double* vy;
    const double* env;
    const uint16_t* vr;
    const uint16_t* slab;
    const int32_t* rects;  // x1, x2, y1, y2 per polygon
    uint32_t npoly;
    int32_t csr;
    int32_t bx0, bx1, by0, by1;
    uint32_t H;
    const uint32_t* cell_off;
    const uint32_t* cell_poly;
    uint8_t* cls;
    unsigned* words;
};

__device__ __forceinline__ bool rect_has(const int32_t* __restrict__ R, int32_t cx, int32_t cy) {
    return cx >= R[0] && cx <= R[1] && cy >= R[2] && cy <= R[3];
}

// The polygon list of cell (cx, cy) as a cursor [cur, end): CSR entries, or polygon numbers to
// test against their rectangles.  False: no polygon's cell set holds the cell.
__device__ __forceinline__ bool cell_list(const TRArgs& a, int32_t cx, int32_t cy, uint32_t& cur, uint32_t& end) {
    if (cx < a.bx0 || cx > a.bx1 || cy < a.by0 || cy > a.by1) return false;
    if (a.csr) {
        const uint32_t k = (uint32_t)(cx - a.bx0) * a.H + (uint32_t)(cy - a.by0);
        cur = a.cell_off[k];
        end = a.cell_off[k + 1];
        return end > cur;
    }
    end = a.npoly;
    for (cur = 0; cur < end; cur++)
        if (rect_has(a.rects + 4 * (size_t)cur, cx, cy)) return true;
    return false;
}

// the next polygon of the list (ascending), kNone at its end
__device__ __forceinline__ uint32_t cell_next(const TRArgs& a, int32_t cx, int32_t cy, uint32_t& cur, uint32_t end) {
    if (a.csr) return cur < end ? a.cell_poly[cur++] : kNone;
    while (cur < end) {
        const uint32_t p = cur++;
        if (rect_has(a.rects + 4 * (size_t)p, cx, cy)) return p;
    }
    return kNone;
}

// the segments count_segment can count or flag for the point: its slab's crossing list, or all
__device__ __forceinline__ void seg_range(const TRArgs& a, const TRPoly& P, double py, uint32_t& k0, uint32_t& k1) {
    if (P.ns) {
        const SlabView sv{a.slab + P.loff, P.ns};
        const uint32_t s = slab_of(py, P.sy0, P.sinv, P.ns);
        k0 = sv.cbeg(s);
        k1 = sv.cbeg(s + 1);
    } else {
        k0 = 0;
        k1 = P.nv - 1;
    }
}

// Is the point (inside the shell's envelope) INTERIOR to polygon P?  PointLocator.locateInPolygon
// from per-ring masks of the rings [64 c, 64 c + 64): bit j of bnd = a segment of ring 64 c + j
// flags the point as on it, bit j of par = odd crossing count.  Shell (chunk 0, bit 0) on the
// boundary or of even parity -> no; a hole with a bit set whose envelope includes the point
// (locateInPolygonRing's envelope test) -> on it or inside it -> no.  WAVE: the 64 lanes hold the
// same point and polygon and split the segments; the masks are reduced across the wave.
template <bool WAVE>
__device__ __forceinline__ bool point_interior(const TRArgs& a, const TRPoly& P, double px, double py, unsigned lane) {
    const double* __restrict__ vx = a.vx + P.voff;
    const double* __restrict__ vy = a.vy + P.voff;
    const uint16_t* __restrict__ vr = a.vr + P.voff;
    const double* __restrict__ env = a.env + 4 * (size_t)P.eoff;
    const SlabView sv{a.slab + P.loff, P.ns};
    uint32_t k0, k1;
    seg_range(a, P, py, k0, k1);
    const bool rings = P.nring > 1;
    const uint32_t nch = (P.nring + 63) / 64;
    for (uint32_t c = 0; c < nch; c++) {
        unsigned long long bnd = 0, par = 0;
        for (uint32_t k = k0 + (WAVE ? lane : 0u); k < k1; k += WAVE ? 64u : 1u) {
            const uint32_t e = P.ns ? sv.id(k) : k;
            uint32_t rid = 0;
            if (rings) {
                rid = vr[e];
                if (vr[e + 1] != rid || (rid >> 6) != c) continue;  // a ring junction is no segment
            }
            bool b = false;
            int cr = 0;
            count_segment(px, py, vx[e + 1], vy[e + 1], vx[e], vy[e], b, cr);
            const unsigned long long bit = 1ull << (rid & 63);
            bnd |= b ? bit : 0ull;
            par ^= (cr & 1) ? bit : 0ull;
        }
        if (WAVE) {
            for (int d = 1; d < 64; d <<= 1) {
                bnd |= __shfl_xor(bnd, d);
                par ^= __shfl_xor(par, d);
            }
        }
        unsigned long long m = bnd | par;
        if (c == 0) {
            if ((bnd & 1ull) || !(par & 1ull)) return false;
            m &= ~1ull;
        }
        while (m) {
            const int h = __builtin_ctzll(m);
            m &= m - 1;
            const double* ev = env + 4 * (64 * (size_t)c + h);
            if (px > ev[2] || px < ev[0] || py > ev[3] || py < ev[1]) continue;
            return false;
        }
    }
    return true;
}

struct WaveQueue {
    double x[kQueue];
    double y[kQueue];
    unsigned idx[kQueue];
    int32_t cx[kQueue];
    int32_t cy[kQueue];
};

// Classes of the queued points [base, base + m), m <= 64, one per lane; the number of class 2.
__device__ __forceinline__ unsigned drain(const TRArgs& a, const WaveQueue& q, unsigned base, unsigned m, unsigned lane) {
    bool active = lane < m;
    double px = 0.0, py = 0.0;
    unsigned idx = 0;
    int32_t cx = 0, cy = 0;
    uint32_t cur = 0, end = 0;
    if (active) {
        px = q.x[base + lane];
        py = q.y[base + lane];
        idx = q.idx[base + lane];
        cx = q.cx[base + lane];
        cy = q.cy[base + lane];
        active = cell_list(a, cx, cy, cur, end);  // true: the point was queued for it
    }
    bool hit = false;
    for (;;) {
        // each lane's next polygon whose envelope covers its point (Geometry.contains' first test)
        uint32_t poly = kNone;
        while (active) {
            const uint32_t p = cell_next(a, cx, cy, cur, end);
            if (p == kNone) {
                active = false;
                break;
            }
            const double* bb = a.polys[p].bb;
            if (px >= bb[0] && px <= bb[2] && py >= bb[1] && py <= bb[3]) {
                poly = p;
                break;
            }
        }
        if (!__ballot(active)) break;
        bool big = false, in = false;
        if (active) {
            const TRPoly& P = a.polys[poly];
            uint32_t k0, k1;
            seg_range(a, P, py, k0, k1);
            big = k1 - k0 > kLaneSegs;
            if (!big) in = point_interior<false>(a, P, px, py, lane);
        }
        unsigned long long bm = __ballot(big);
        while (bm) {
            const int src = __builtin_ctzll(bm);
            bm &= bm - 1;
            const uint32_t wp = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(poly, src));
            const double wx = __shfl(px, src), wy = __shfl(py, src);
            const bool r = point_interior<true>(a, a.polys[wp], wx, wy, lane);
            if ((int)lane == src) in = r;
        }
        if (active && in) {  // a point stops at the first polygon that contains it
            hit = true;
            active = false;
        }
    }
    if (lane < m) a.cls[idx] = hit ? 2 : 1;
    return (unsigned)__popcll(__ballot(hit));
}

__global__ void __launch_bounds__(kTB) trange_classify(TRArgs a) {
    __shared__ WaveQueue queue[kWaves];
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    WaveQueue& q = queue[wave];
    unsigned qn = 0, hits = 0;  // wave-uniform
    const uint64_t nbatch = (a.n + 63) / 64;
    // a wave takes runs of kWaveBatches consecutive batches, so that its queue fills across batches
    // and most drains are full ones, whatever the share of queued points
    const uint64_t nrun = (nbatch + kWaveBatches - 1) / kWaveBatches;
    const uint64_t nwave = (uint64_t)gridDim.x * kWaves;
    // batch t of this wave's sequence: run (first + t / kWaveBatches * nwave), batch t % kWaveBatches of it
    for (uint64_t t = 0;; t++) {
        const uint64_t r = (uint64_t)blockIdx.x * kWaves + wave + t / kWaveBatches * nwave;
        if (r >= nrun) break;
        const uint64_t b = r * kWaveBatches + t % kWaveBatches;
        if (b >= nbatch) break;  // the last run may be short
        const uint64_t i = b * 64 + lane;
        bool cand = false;
        double px = 0.0, py = 0.0;
        int32_t cx = 0, cy = 0;
        if (i < a.n) {
            px = a.x[i];
            py = a.y[i];
            cx = d_axis_cell(px, a.mnx, a.l);
            cy = d_axis_cell(py, a.mny, a.l);
            uint32_t cur, end;
            cand = cell_list(a, cx, cy, cur, end);
            if (!cand) a.cls[i] = 0;
        }
        const unsigned long long cm = __ballot(cand);
        if (cm) {
            if (cand) {
                const unsigned at = qn + lanes_below(cm);  // < 64 + 64
                q.x[at] = px;
                q.y[at] = py;
                q.idx[at] = (unsigned)i;
                q.cx[at] = cx;
                q.cy[at] = cy;
            }
            qn += (unsigned)__popcll(cm);
            wave_lds_sync();
            if (qn >= 64) {
                hits += drain(a, q, qn - 64, 64, lane);
                qn -= 64;
                wave_lds_sync();  // the drained entries are read before the next batch overwrites them
            }
        }
    }
    if (qn) hits += drain(a, q, 0, qn, lane);
    if (lane == 0 && hits) atomicAdd(&a.words[1], hits);
}

struct IsContained {
    const uint8_t* cls;
    __device__ bool operator()(unsigned i) const { return cls[i] == 2; }
};

// ---- hit filter -------------------------------------------------------------------------------
// flag[t] = 1 for the trajectory of every point at or above the threshold (equal stores)
__global__ void __launch_bounds__(kTB) hit_mark(const unsigned* __restrict__ traj_of, const uint8_t* __restrict__ cls,
                                                unsigned n, unsigned T, unsigned threshold, unsigned* __restrict__ flag,
                                                unsigned* __restrict__ words) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const unsigned t = traj_of[i];
    if (t == kNone) return;
    if (t >= T) {
        atomicOr(&words[0], kErrIndex);
        return;
    }
    if (cls[i] >= threshold) flag[t] = 1u;
}

// len[t] = the points of a marked trajectory (t <= T; flag[T] = len[T] = 0 carry the totals
// through the exclusive scans)
__global__ void __launch_bounds__(kTB) hit_lengths(const unsigned* __restrict__ traj_off, unsigned T, unsigned n_sel,
                                                   unsigned* __restrict__ flag, unsigned* __restrict__ len,
                                                   unsigned* __restrict__ words) {
    const unsigned t = blockIdx.x * kTB + threadIdx.x;
    if (t > T) return;
    unsigned v = 0;
    if (t < T) {
        const unsigned b = traj_off[t], e = traj_off[t + 1];
        if (e < b || e > n_sel) atomicOr(&words[0], kErrIndex);
        else if (flag[t]) v = e - b;
    } else {
        flag[T] = 0u;
    }
    len[t] = v;
}

__global__ void __launch_bounds__(kTB) hit_trajs(const unsigned* __restrict__ flag, const unsigned* __restrict__ newid,
                                                 const unsigned* __restrict__ newoff, const unsigned* __restrict__ traj_first,
                                                 unsigned T, unsigned* __restrict__ out_first, unsigned* __restrict__ out_off,
                                                 unsigned* __restrict__ hit_traj) {
    const unsigned t = blockIdx.x * kTB + threadIdx.x;
    if (t > T) return;
    if (t == T) {
        out_off[newid[T]] = newoff[T];  // newid[T] = T' <= T
        return;
    }
    if (!flag[t]) return;
    const unsigned u = newid[t];
    out_first[u] = traj_first[t];
    out_off[u] = newoff[t];
    hit_traj[u] = t;
}

__global__ void __launch_bounds__(kTB) hit_points(const unsigned* __restrict__ traj_of, const unsigned* __restrict__ flag,
                                                  const unsigned* __restrict__ newid, unsigned n,
                                                  unsigned* __restrict__ out_traj_of) {
    const unsigned i = blockIdx.x * kTB + threadIdx.x;
    if (i >= n) return;
    const unsigned t = traj_of[i];  // hit_mark checked t < T
    out_traj_of[i] = t != kNone && flag[t] ? newid[t] : kNone;
}

// perm[j] belongs to trajectory traj_of[perm[j]], whose slice must hold j: then its place in the
// new slice is newoff[t] + (j - traj_off[t]) < newoff[t] + len[t] <= n_hit_sel
__global__ void __launch_bounds__(kTB) hit_perm(const unsigned* __restrict__ perm, const unsigned* __restrict__ traj_of,
                                                const unsigned* __restrict__ traj_off, const unsigned* __restrict__ flag,
                                                const unsigned* __restrict__ newoff, unsigned n, unsigned n_sel,
                                                unsigned* __restrict__ out_perm, unsigned* __restrict__ words) {
    const unsigned j = blockIdx.x * kTB + threadIdx.x;
    if (j >= n_sel) return;
    const unsigned p = perm[j];
    if (p >= n) {
        atomicOr(&words[0], kErrIndex);
        return;
    }
    const unsigned t = traj_of[p];
    if (t == kNone || j < traj_off[t] || j >= traj_off[t + 1]) {
        atomicOr(&words[0], kErrIndex);
        return;
    }
    if (flag[t]) out_perm[newoff[t] + (j - traj_off[t])] = p;
}

// ---- host side --------------------------------------------------------------------------------
// The ctx's plan of its last polygon set: a continuous query classifies every window against the
// same polygons, so the host planning and the upload happen once; later calls compare their
// inputs bitwise with the cached copies.
struct TRangeCache {
    uint64_t budget = kTRangeCellBudget;  // geohip_debug_trange_cell_budget
    bool valid = false;
    geohip_grid grid{};
    uint64_t plan_budget = 0;
    bool had_rings = false;
    std::vector<uint32_t> poly_rings, ring_off;
    std::vector<double> vx, vy;
    // the device tables, one allocation: TRPoly[] | vx | vy | env | rects | cell_off | cell_poly | vr | slabs
    void* dev = nullptr;
    size_t off_vx = 0, off_vy = 0, off_env = 0, off_rect = 0, off_co = 0, off_cp = 0, off_vr = 0, off_slab = 0;
    uint32_t npoly = 0;
    bool csr = false;
    int32_t bx0 = 0, bx1 = -1, by0 = 0, by1 = -1;
};

TRangeCache* ctx_tcache(geohip_ctx* ctx) {
    void** slot = ctx_tcache_slot(ctx);
    if (!*slot) *slot = new TRangeCache();
    return static_cast<TRangeCache*>(*slot);
}

bool same_polygons(const TRangeCache& c, const geohip_grid& g, const uint32_t* poly_rings, const uint32_t* ring_off,
                   const double* vx, const double* vy, uint32_t npoly) {
    if (!c.valid || c.plan_budget != c.budget || c.npoly != npoly) return false;
    if (c.grid.min_x != g.min_x || c.grid.min_y != g.min_y || c.grid.cell_len != g.cell_len || c.grid.n != g.n) return false;
    if (c.had_rings != (poly_rings != nullptr)) return false;
    if (poly_rings && memcmp(c.poly_rings.data(), poly_rings, ((size_t)npoly + 1) * 4) != 0) return false;
    const uint32_t R0 = poly_rings ? poly_rings[0] : 0, R1 = poly_rings ? poly_rings[npoly] : npoly;
    if (R1 < R0 || c.ring_off.size() != (size_t)(R1 - R0) + 1) return false;
    if (memcmp(c.ring_off.data(), ring_off + R0, ((size_t)(R1 - R0) + 1) * 4) != 0) return false;
    const size_t v0 = ring_off[R0], v1 = ring_off[R1];
    if (v1 < v0 || c.vx.size() != v1 - v0) return false;
    return memcmp(c.vx.data(), vx + v0, (v1 - v0) * 8) == 0 && memcmp(c.vy.data(), vy + v0, (v1 - v0) * 8) == 0;
}

// y-slab crossing lists of one polygon in SlabView's layout (the distance lists stay empty),
// appended to blob; P.ns = 0 when they cannot be built (few or very many segments, no finite
// extent): the device then visits every segment.  slab_of is monotone in y, so a segment that
// count_segment can count or flag for a point (lo <= py <= hi) is in the point's slab list.
void plan_crossing_slabs(TRPoly& P, const double* ry, const uint16_t* rid, const double* env, std::vector<uint16_t>& blob) {
    P.ns = 0;
    P.sy0 = 0.0;
    P.sinv = 0.0;
    P.loff = (uint32_t)blob.size();
    const uint32_t nseg = P.nv >= 2 ? P.nv - 1 : 0;
    if (nseg < 8 || nseg > 30000) return;
    double y0 = env[1], y1 = env[3];
    for (uint32_t j = 1; j < P.nring; j++) {
        y0 = std::min(y0, env[4 * j + 1]);
        y1 = std::max(y1, env[4 * j + 3]);
    }
    const uint32_t ns = std::min<uint32_t>(64, nseg);
    const double span = y1 - y0;
    if (!(span > 0.0) || !std::isfinite(span) || !std::isfinite(y0)) return;
    const double sinv = (double)ns / span;
    if (!(sinv > 0.0) || !std::isfinite(sinv)) return;
    const double pad = 1e-6 * span / ns;
    auto range = [&](uint32_t e, uint32_t& c0, uint32_t& c1) -> bool {
        const double a = ry[e], b = ry[e + 1];
        if (a != a || b != b) return false;  // a NaN y never counts or flags
        if (rid[e] != rid[e + 1]) return false;
        c0 = slab_of(std::min(a, b) - pad, y0, sinv, ns);
        c1 = slab_of(std::max(a, b) + pad, y0, sinv, ns);
        return true;
    };
    uint32_t cn[65] = {0};
    uint64_t total = 0;
    for (uint32_t e = 0; e < nseg; e++) {
        uint32_t c0, c1;
        if (!range(e, c0, c1)) continue;
        for (uint32_t t = c0; t <= c1; t++) cn[t]++;
        total += c1 - c0 + 1;
    }
    if (total + 2ull * (ns + 1) > 65535ull || blob.size() + 2ull * (ns + 1) + total >= 0xffffffffull) return;
    const size_t h = blob.size();
    blob.resize(h + 2 * (ns + 1) + total);
    uint16_t* B = blob.data() + h;
    uint32_t k = 0;
    for (uint32_t t = 0; t < ns; t++) { B[t] = (uint16_t)k; k += cn[t]; }
    B[ns] = (uint16_t)k;
    for (uint32_t t = 0; t <= ns; t++) B[ns + 1 + t] = (uint16_t)k;
    uint32_t cf[64] = {0};
    uint16_t* ids = B + 2 * (ns + 1);
    for (uint32_t e = 0; e < nseg; e++) {
        uint32_t c0, c1;
        if (!range(e, c0, c1)) continue;
        for (uint32_t t = c0; t <= c1; t++) ids[B[t] + cf[t]++] = (uint16_t)e;
    }
    P.ns = ns;
    P.sy0 = y0;
    P.sinv = sinv;
}

inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// plan and upload the polygon set unless it is the cached one
int prepare_polygons(geohip_ctx* ctx, const geohip_grid& g, const uint32_t* poly_rings, const uint32_t* ring_off,
                     const double* vx, const double* vy, uint64_t nv, uint32_t npoly, TRangeCache** out) {
    TRangeCache* c = ctx_tcache(ctx);
    *out = c;
    // the cheap argument checks come first: same_polygons reads the arrays through them
    for (uint32_t p = 0; p < npoly && poly_rings; p++)
        if (poly_rings[p + 1] <= poly_rings[p])
            return ctx_fail(ctx, GEOHIP_ERR_ARG, "poly_rings not strictly ascending (a polygon needs a ring)");
    const uint32_t R0 = poly_rings ? poly_rings[0] : 0, R1 = poly_rings ? poly_rings[npoly] : npoly;
    for (uint32_t j = R0; j < R1; j++)
        if (ring_off[j + 1] < ring_off[j]) return ctx_fail(ctx, GEOHIP_ERR_ARG, "ring_off not ascending");
    if (ring_off[R1] > nv) return ctx_fail(ctx, GEOHIP_ERR_ARG, "ring_off refers past the nv vertices of vx / vy");
    if (same_polygons(*c, g, poly_rings, ring_off, vx, vy, npoly)) return GEOHIP_OK;
    c->valid = false;
    TRangePlan pl;
    std::string err;
    int rc = plan_trange(g, poly_rings, ring_off, vx, vy, nv, npoly, c->budget, nullptr, &pl, &err);
    if (rc) return ctx_fail(ctx, rc, err);
    std::vector<TRPoly> dp(npoly);
    std::vector<uint16_t> slabs;
    std::vector<int32_t> rects(4 * (size_t)npoly);
    for (uint32_t p = 0; p < npoly; p++) {
        const TRangePolygon& S = pl.polys[p];
        TRPoly& P = dp[p];
        memset(&P, 0, sizeof P);
        memcpy(P.bb, S.bb, sizeof P.bb);
        P.voff = S.voff;
        P.nv = S.nv;
        P.nring = S.nring;
        P.eoff = S.eoff;
        memcpy(&rects[4 * (size_t)p], S.rect, sizeof S.rect);
        plan_crossing_slabs(P, pl.vy.data() + S.voff, pl.vr.data() + S.voff, pl.env.data() + 4 * (size_t)S.eoff, slabs);
    }
    const size_t sz_p = dp.size() * sizeof(TRPoly), sz_v = pl.vx.size() * 8, sz_e = pl.env.size() * 8;
    const size_t sz_r = rects.size() * 4, sz_co = pl.cell_off.size() * 4, sz_cp = pl.cell_poly.size() * 4;
    const size_t sz_vr = pl.vr.size() * 2, sz_s = slabs.size() * 2;
    c->off_vx = align16(sz_p);
    c->off_vy = align16(c->off_vx + sz_v);
    c->off_env = align16(c->off_vy + sz_v);
    c->off_rect = align16(c->off_env + sz_e);
    c->off_co = align16(c->off_rect + sz_r);
    c->off_cp = align16(c->off_co + sz_co);
    c->off_vr = align16(c->off_cp + sz_cp);
    c->off_slab = align16(c->off_vr + sz_vr);
    const size_t total = align16(c->off_slab + sz_s) + 64;
    std::vector<char> host(total, 0);
    memcpy(host.data(), dp.data(), sz_p);
    memcpy(host.data() + c->off_vx, pl.vx.data(), sz_v);
    memcpy(host.data() + c->off_vy, pl.vy.data(), sz_v);
    memcpy(host.data() + c->off_env, pl.env.data(), sz_e);
    memcpy(host.data() + c->off_rect, rects.data(), sz_r);
    if (sz_co) memcpy(host.data() + c->off_co, pl.cell_off.data(), sz_co);
    if (sz_cp) memcpy(host.data() + c->off_cp, pl.cell_poly.data(), sz_cp);
    memcpy(host.data() + c->off_vr, pl.vr.data(), sz_vr);
    if (sz_s) memcpy(host.data() + c->off_slab, slabs.data(), sz_s);
    hipStream_t st = ctx_stream(ctx);
    if (c->dev) {
        GEOHIP_CHK(hipStreamSynchronize(st));  // the previous call's kernel may still read the old tables
        GEOHIP_CHK(hipFree(c->dev));
        c->dev = nullptr;
    }
    if (hipMalloc(&c->dev, total) != hipSuccess) {
        c->dev = nullptr;
        return ctx_fail(ctx, GEOHIP_ERR_OOM, "polygon tables: out of device memory");
    }
    GEOHIP_CHK(hipMemcpyAsync(c->dev, host.data(), total, hipMemcpyHostToDevice, st));
    GEOHIP_CHK(hipStreamSynchronize(st));  // host is a local
    c->grid = g;
    c->plan_budget = c->budget;
    c->npoly = npoly;
    c->had_rings = poly_rings != nullptr;
    if (poly_rings) c->poly_rings.assign(poly_rings, poly_rings + npoly + 1);
    else c->poly_rings.clear();
    c->ring_off.assign(ring_off + R0, ring_off + R1 + 1);
    c->vx.assign(vx + ring_off[R0], vx + ring_off[R1]);
    c->vy.assign(vy + ring_off[R0], vy + ring_off[R1]);
    c->csr = pl.csr;
    c->bx0 = pl.bx0; c->bx1 = pl.bx1; c->by0 = pl.by0; c->by1 = pl.by1;
    c->valid = true;
    return GEOHIP_OK;
}

}  // namespace

void trange_cache_drop(geohip_ctx* ctx) {
    void** slot = ctx_tcache_slot(ctx);
    TRangeCache* c = static_cast<TRangeCache*>(*slot);
    if (c && c->dev) hipFree(c->dev);
    delete c;
    *slot = nullptr;
}

}  // namespace geohip

using namespace geohip;

extern "C" {

int geohip_trange_classify(geohip_ctx* ctx, const geohip_grid* grid, const double* x, const double* y, uint64_t n,
                           const uint32_t* poly_rings, const uint32_t* ring_off, const double* vx, const double* vy,
                           uint64_t nv, uint32_t npoly, uint8_t* out_class, uint32_t* out_idx, uint64_t cap,
                           uint64_t* out_count) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!out_count) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out_count");
    *out_count = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_trange_classify takes device memory");
    if (!grid) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null grid");
    if (n >= 0xffffffffull) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "window larger than 2^32-1 points");
    if (cap && !out_idx) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null out_idx");
    if (n && (!x || !y || !out_class)) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    if (npoly == 0) {  // no polygon, no cell: every class is 0 (the polygon arrays may be null)
        std::string err;
        rc = plan_trange(*grid, nullptr, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, &err);  // the grid's checks
        if (rc) return ctx_fail(ctx, rc, err);
        if (n) GEOHIP_CHK(hipMemsetAsync(out_class, 0, n, st));
        return GEOHIP_OK;
    }
    if (!ring_off || !vx || !vy) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null polygon arrays");
    TRangeCache* c = nullptr;
    rc = prepare_polygons(ctx, *grid, poly_rings, ring_off, vx, vy, nv, npoly, &c);
    if (rc) return rc;
    if (n == 0) return GEOHIP_OK;
    unsigned* words;
    rc = scratch<R_WORDS>(ctx, 64, &words);
    if (rc) return rc;
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    const char* d = static_cast<const char*>(c->dev);
    TRArgs a;
    memset(&a, 0, sizeof a);
    a.x = x;
    a.y = y;
    a.n = n;
    a.mnx = grid->min_x;
    a.mny = grid->min_y;
    a.l = grid->cell_len;
    a.polys = reinterpret_cast<const TRPoly*>(d);
    a.vx = reinterpret_cast<const double*>(d + c->off_vx);
    a.vy = reinterpret_cast<const double*>(d + c->off_vy);
    a.env = reinterpret_cast<const double*>(d + c->off_env);
    a.rects = reinterpret_cast<const int32_t*>(d + c->off_rect);
    a.cell_off = reinterpret_cast<const uint32_t*>(d + c->off_co);
    a.cell_poly = reinterpret_cast<const uint32_t*>(d + c->off_cp);
    a.vr = reinterpret_cast<const uint16_t*>(d + c->off_vr);
    a.slab = reinterpret_cast<const uint16_t*>(d + c->off_slab);
    a.npoly = npoly;
    a.csr = c->csr ? 1 : 0;
    a.bx0 = c->bx0; a.bx1 = c->bx1; a.by0 = c->by0; a.by1 = c->by1;
    a.H = c->by1 >= c->by0 ? (uint32_t)(c->by1 - c->by0 + 1) : 0u;
    a.cls = out_class;
    a.words = words;
    // a persistent grid of exactly the resident blocks: a block beyond them would start its equal
    // share of the batches only after another has finished
    static const int resident = [] {
        int nb = 0;
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, trange_classify, kTB, 0) == hipSuccess && nb > 0 ? nb : 4;
    }();
    const uint64_t runs = ((n + 63) / 64 + kWaveBatches - 1) / kWaveBatches;
    const uint64_t want = (runs + kWaves - 1) / kWaves;
    const unsigned grid_blocks = (unsigned)std::min<uint64_t>(want, (uint64_t)ctx_cus(ctx) * (uint64_t)resident);
    tlaunch(ctx, trange_classify, dim3(grid_blocks), dim3(kTB), 0, st, a);
    GEOHIP_CHK(hipGetLastError());
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 8, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    const uint64_t count = pin[0] >> 32;
    *out_count = count;
    if (!out_idx && cap == 0) return GEOHIP_OK;  // classes only
    if (count > cap) return ctx_fail(ctx, GEOHIP_ERR_CAPACITY, "output capacity too small; *out_count = required");
    if (count == 0) return GEOHIP_OK;
    // the class-2 indices, ascending: count <= cap of them are written
    const rocprim::counting_iterator<unsigned> iota(0u);
    const IsContained pred{out_class};
    size_t tb = 0;
    GEOHIP_CHK(rocprim::select(nullptr, tb, iota, out_idx, (unsigned*)nullptr, n, pred, st));
    void* temp;
    rc = scratch<R_TEMP>(ctx, tb + 16, &temp);
    if (rc) return rc;
    GEOHIP_CHK(rocprim::select(temp, tb, iota, out_idx, words + 2, n, pred, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    return GEOHIP_OK;
}

// Test hook: the cell budget of this ctx's cell -> polygon CSR (0: kTRangeCellBudget).  With a
// budget below the polygons' bounding rectangle the rectangle-scan path runs.
int geohip_debug_trange_cell_budget(geohip_ctx* ctx, uint64_t cells) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    ctx_tcache(ctx)->budget = cells ? cells : kTRangeCellBudget;
    return GEOHIP_OK;
}

int geohip_traj_filter_hit(geohip_ctx* ctx, const uint32_t* traj_of, const uint32_t* traj_first, const uint32_t* traj_off,
                           const uint32_t* perm, uint64_t n, uint64_t n_traj, uint64_t n_sel, const uint8_t* cls,
                           uint32_t threshold, uint32_t* out_traj_of, uint32_t* out_traj_first, uint32_t* out_traj_off,
                           uint32_t* out_perm, uint32_t* hit_traj, uint64_t* n_hit_traj, uint64_t* n_hit_sel) {
    int rc = ctx_begin(ctx);
    if (rc) return rc;
    if (!n_hit_traj || !n_hit_sel) return ctx_fail(ctx, GEOHIP_ERR_ARG, "null n_hit_traj / n_hit_sel");
    *n_hit_traj = 0;
    *n_hit_sel = 0;
    if (ctx_mem(ctx) != GEOHIP_MEM_DEVICE) return ctx_fail(ctx, GEOHIP_ERR_ARG, "geohip_traj_filter_hit takes device memory");
    if (n > kMaxPoints || n_sel > kMaxPoints || n_traj > kMaxPoints) return ctx_fail(ctx, GEOHIP_ERR_UNSUPPORTED, "more than 2^30 points");
    if (n_sel > n || n_traj > n_sel) return ctx_fail(ctx, GEOHIP_ERR_ARG, "n_traj <= n_sel <= n does not hold");
    if (!out_traj_off || (n && (!traj_of || !cls || !out_traj_of)) ||
        (n_traj && (!traj_first || !traj_off || !perm || !out_traj_first || !out_perm || !hit_traj)))
        return ctx_fail(ctx, GEOHIP_ERR_ARG, "null argument");
    hipStream_t st = ctx_stream(ctx);
    const unsigned nn = (unsigned)n, T = (unsigned)n_traj, ns = (unsigned)n_sel;
    if (T == 0) {
        GEOHIP_CHK(hipMemsetAsync(out_traj_off, 0, 4, st));
        if (n) GEOHIP_CHK(hipMemsetAsync(out_traj_of, 0xff, n * 4, st));
        return GEOHIP_OK;
    }
    size_t tb = 0;
    GEOHIP_CHK(rocprim::exclusive_scan(nullptr, tb, (unsigned*)nullptr, (unsigned*)nullptr, 0u, (size_t)T + 1,
                                       rocprim::plus<unsigned>(), st));
    unsigned *flag, *newid, *len, *newoff, *words;
    void* temp;
    const size_t tw = ((size_t)T + 1) * 4;
    rc = scratch<R_FLAG>(ctx, tw, &flag);
    if (!rc) rc = scratch<R_NEWID>(ctx, tw, &newid);
    if (!rc) rc = scratch<R_LEN>(ctx, tw, &len);
    if (!rc) rc = scratch<R_NEWOFF>(ctx, tw, &newoff);
    if (!rc) rc = scratch<R_TEMP>(ctx, tb + 16, &temp);
    if (!rc) rc = scratch<R_WORDS>(ctx, 64, &words);
    if (rc) return rc;
    GEOHIP_CHK(hipMemsetAsync(flag, 0, tw, st));
    GEOHIP_CHK(hipMemsetAsync(words, 0, 64, st));
    tlaunch(ctx, hit_mark, dim3(blocks_for(n)), dim3(kTB), 0, st, traj_of, cls, nn, T, (unsigned)threshold, flag, words);
    tlaunch(ctx, hit_lengths, dim3(blocks_for((uint64_t)T + 1)), dim3(kTB), 0, st, traj_off, T, ns, flag, len, words);
    size_t tb2 = tb;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb2, flag, newid, 0u, (size_t)T + 1, rocprim::plus<unsigned>(), st));
    tb2 = tb;
    GEOHIP_CHK(rocprim::exclusive_scan(temp, tb2, len, newoff, 0u, (size_t)T + 1, rocprim::plus<unsigned>(), st));
    uint64_t* pin = ctx_pinned(ctx);
    GEOHIP_CHK(hipGetLastError());
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipMemcpyAsync(pin + 1, newid + T, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipMemcpyAsync(pin + 2, newoff + T, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    const char* bad = "geohip_traj_filter_hit: traj_of entry >= n_traj, perm entry >= n or outside its trajectory's "
                      "slice, or traj_off not ascending or past n_sel";
    if ((pin[0] & 0xffffffffu) & kErrIndex) return ctx_fail(ctx, GEOHIP_ERR_ARG, bad);
    const unsigned Th = (unsigned)(pin[1] & 0xffffffffu), nh = (unsigned)(pin[2] & 0xffffffffu);
    tlaunch(ctx, hit_trajs, dim3(blocks_for((uint64_t)T + 1)), dim3(kTB), 0, st, (const unsigned*)flag,
            (const unsigned*)newid, (const unsigned*)newoff, traj_first, T, out_traj_first, out_traj_off, hit_traj);
    if (nn)
        tlaunch(ctx, hit_points, dim3(blocks_for(n)), dim3(kTB), 0, st, traj_of, (const unsigned*)flag,
                (const unsigned*)newid, nn, out_traj_of);
    if (ns)
        tlaunch(ctx, hit_perm, dim3(blocks_for(n_sel)), dim3(kTB), 0, st, perm, traj_of, traj_off, (const unsigned*)flag,
                (const unsigned*)newoff, nn, ns, out_perm, words);
    GEOHIP_CHK(hipGetLastError());
    GEOHIP_CHK(hipMemcpyAsync(pin, words, 4, hipMemcpyDeviceToHost, st));
    GEOHIP_CHK(hipStreamSynchronize(st));
    if ((pin[0] & 0xffffffffu) & kErrIndex) return ctx_fail(ctx, GEOHIP_ERR_ARG, bad);
    *n_hit_traj = Th;
    *n_hit_sel = nh;
    return GEOHIP_OK;
}

}  // extern "C"
