// locate.h -- device pieces shared by the cell kernels (cell_kernels.hip, trange.hip, tagg.hip,
// tjoin.hip): a point's grid cell, the neighbour square of a join's query point with its cell
// key's round trip through Java, RayCrossingCounter.countSegment with the exact determinant sign,
// and the y-slab crossing lists of a planned polygon.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_common.h"

namespace geohip {

__device__ __forceinline__ int32_t d_java_d2i(double v) {
    if (v != v) return 0;
    if (v >= 2147483647.0) return INT32_MAX;
    if (v <= -2147483648.0) return INT32_MIN;
    return (int32_t)v;
}

// HelperClass.assignGridCellID per axis: (int)Math.floor((v - min)/l), exact division.
__device__ __forceinline__ int32_t d_axis_cell(double v, double mn, double l) {
    return d_java_d2i(__builtin_floor((v - mn) / l));
}

// A cell key's round trip through Java, as both joins replicate their query points (jq_rect in
// cell_kernels.hip, tj_qrect in tjoin.hip).  The key is String.format("%05d", cx) +
// String.format("%05d", cy) (HelperClass.java:54-57, 117-120); getIntCellIndices
// (HelperClass.java:263-276) splits it after the fifth character and reads each half with
// Integer.parseInt(s.replaceFirst("^0+(?!$)", "")) (HelperClass.java:60-63).  A cell outside
// [-9999, 99999] makes a key that is not 10 characters, so the split lands elsewhere.
__device__ __forceinline__ int d_format05(int32_t v, char* out) {
    char digits[12];
    int nd = 0;
    int64_t a = v;
    const bool neg = a < 0;
    if (neg) a = -a;
    do {
        digits[nd++] = (char)('0' + (int)(a % 10));
        a /= 10;
    } while (a != 0);
    const int width = nd + (neg ? 1 : 0);
    int p = 0;
    if (neg) out[p++] = '-';
    for (int i = width; i < 5; i++) out[p++] = '0';
    while (nd > 0) out[p++] = digits[--nd];
    return p;
}
__device__ __forceinline__ bool d_java_parse(const char* s, int len, int32_t* out) {
    int skip = 0;
    while (skip < len - 1 && s[skip] == '0') skip++;
    s += skip;
    len -= skip;
    if (len <= 0) return false;
    bool neg = false;
    int p = 0;
    if (s[0] == '+' || s[0] == '-') {
        if (len == 1) return false;
        neg = s[0] == '-';
        p = 1;
    }
    int64_t v = 0;
    for (; p < len; p++) {
        if (s[p] < '0' || s[p] > '9') return false;
        v = v * 10 + (s[p] - '0');
        if (v > 2147483648LL) return false;
    }
    if (neg) v = -v;
    if (v > INT32_MAX || v < INT32_MIN) return false;
    *out = (int32_t)v;
    return true;
}

struct QRect {
    int32_t x0, x1, y0, y1;  // cells, clipped; x0 > x1 = empty
};

// UniformGrid.getNeighboringCells (UniformGrid.java:261-293) of a point whose unclipped cell is
// (cx, cy): the cell indices as its key hands them on, the int-wrapping loops [c - lc, c + lc] on
// both axes, and of their cells those inside [0, nside - 1].  Returns 0 with R the clipped square
// (empty where a wrapped loop runs no step); 1 = the key does not parse (NumberFormatException) and
// 2 = a loop's bound is Integer.MAX_VALUE, so it never ends -- both with R empty.
__device__ __forceinline__ int d_neighbor_square(int32_t cx, int32_t cy, int32_t lc, int32_t nside, QRect& R) {
    int32_t ci = cx, cj = cy;
    bool ok = true;
    if (!(cx >= -9999 && cx <= 99999 && cy >= -9999 && cy <= 99999)) {
        char key[24];
        int n = d_format05(cx, key);
        n += d_format05(cy, key + n);
        ok = d_java_parse(key, 5, &ci) && d_java_parse(key + 5, n - 5, &cj);
    }
    R = QRect{1, 0, 1, 0};
    if (!ok) return 1;
    const int32_t lo_i = (int32_t)(uint32_t)(uint64_t)((int64_t)ci - lc);
    const int32_t hi_i = (int32_t)(uint32_t)(uint64_t)((int64_t)ci + lc);
    const int32_t lo_j = (int32_t)(uint32_t)(uint64_t)((int64_t)cj - lc);
    const int32_t hi_j = (int32_t)(uint32_t)(uint64_t)((int64_t)cj + lc);
    if (lo_i > hi_i || lo_j > hi_j) return 0;
    if (hi_i == INT32_MAX || hi_j == INT32_MAX) return 2;
    R = QRect{lo_i > 0 ? lo_i : 0, hi_i < nside - 1 ? hi_i : nside - 1, lo_j > 0 ? lo_j : 0, hi_j < nside - 1 ? hi_j : nside - 1};
    return 0;
}

// Exact sign of x1*y2 - y1*x2 (RobustDeterminant.signOfDet2x2): error-free products by fma,
// summed as a Shewchuk expansion; the most significant nonzero component carries the sign.
__device__ __forceinline__ void two_sum(double a, double b, double& s, double& e) {
    s = a + b;
    const double bv = s - a;
    const double av = s - bv;
    e = (a - av) + (b - bv);
}

// fma(a, b, -fl(a b)) is the product's rounding error only while that error is representable and
// nothing overflowed: |a b| in [2^-960, 2^1020], or an exact zero.
__device__ __forceinline__ bool product_error_free(double a, double b, double p) {
    const double ap = __builtin_fabs(p);
    return (ap >= 0x1.0p-960 && ap <= 0x1.0p1020) || a == 0.0 || b == 0.0;
}
__device__ __forceinline__ int exact_det_sign_normal(double x1, double y1, double x2, double y2);

// The same sign when a product leaves that range (finite operands): with v = m_v 2^e_v (frexp,
// |m_v| in [1/2, 1)) the products are (m_x1 m_y2) 2^(a + b) and (m_y1 m_x2) 2^(c + d), the
// mantissa products in [1/4, 1).  Different signs or an exponent gap of 3 decide; otherwise one
// operand takes the gap (an exact scaling by at most 4) and the expansion runs on the mantissas,
// whose products and residuals are normal.  RobustDeterminant forms no product at all, so its
// answer is the exact sign whatever the magnitudes.
__device__ __noinline__ int exact_det_sign_scaled(double x1, double y1, double x2, double y2) {
    int a, b, c, d;
    double mx1 = __builtin_frexp(x1, &a);
    const double my2 = __builtin_frexp(y2, &b);
    double my1 = __builtin_frexp(y1, &c);
    const double mx2 = __builtin_frexp(x2, &d);
    const double mp = mx1 * my2, mq = my1 * mx2;
    const int sp = (mp > 0.0) - (mp < 0.0), sq = (mq > 0.0) - (mq < 0.0);
    if (sp != sq) return sp > sq ? 1 : -1;
    if (sp == 0) return 0;
    const int de = (a + b) - (c + d);
    if (de >= 3) return sp;
    if (de <= -3) return -sp;
    if (de >= 0) mx1 = __builtin_ldexp(mx1, de);
    else my1 = __builtin_ldexp(my1, -de);
    return exact_det_sign_normal(mx1, my1, mx2, my2);
}

__device__ __forceinline__ int exact_det_sign(double x1, double y1, double x2, double y2) {
    const double p0 = x1 * y2, q0 = y1 * x2;
    if (!(product_error_free(x1, y2, p0) && product_error_free(y1, x2, q0)) &&
        __builtin_fabs(x1) <= kDblMax && __builtin_fabs(y1) <= kDblMax && __builtin_fabs(x2) <= kDblMax &&
        __builtin_fabs(y2) <= kDblMax)
        return exact_det_sign_scaled(x1, y1, x2, y2);
    return exact_det_sign_normal(x1, y1, x2, y2);
}

__device__ __forceinline__ int exact_det_sign_normal(double x1, double y1, double x2, double y2) {
    const double p = x1 * y2;
    const double ep = __builtin_fma(x1, y2, -p);
    const double q = y1 * x2;
    const double eq = __builtin_fma(y1, x2, -q);
    // grow [ep, p] by -eq, then by -q
    double h0, h1, h2, h3, Q, t;
    two_sum(-eq, ep, Q, h0);
    two_sum(Q, p, t, h1);
    Q = t;
    h2 = Q;  // expansion [h0, h1, h2]
    double g0, g1, g2;
    two_sum(-q, h0, Q, g0);
    two_sum(Q, h1, t, g1);
    Q = t;
    two_sum(Q, h2, t, g2);
    h3 = t;  // [g0, g1, g2, h3]
    if (h3 != 0) return h3 > 0 ? 1 : -1;
    if (g2 != 0) return g2 > 0 ? 1 : -1;
    if (g1 != 0) return g1 > 0 ? 1 : -1;
    if (g0 != 0) return g0 > 0 ? 1 : -1;
    return 0;
}

// Polygons with holes: rings are stored back to back in one vertex run, with a ring id per
// vertex (u16, < kMaxRings); segment (v[e], v[e+1]) exists iff both ends carry the same id (the
// junction between two rings is not an edge).  Crossing parity and boundary flags are kept per
// ring as 64-bit masks over a chunk of 64 rings (ring = 64 c + bit), so segments may still be
// visited in any order; a polygon of more than 64 rings takes one pass per chunk until a chunk
// decides (rings_locate_chunk).
constexpr uint32_t kMaxRings = 65535;
typedef uint16_t ring_id_t;

// A polygon's y-slab index (u16): cbeg[ns + 1] | dbeg[ns + 1] | segment ids.  Crossing list of
// slab s: segments (v[e], v[e+1]) whose y-range meets the slab (padded) -- every segment that
// RayCrossingCounter.countSegment can count or flag for a point whose y falls in the slab.
// Distance list: segments whose y-range widened by E meets the slab; a point whose screen
// radius is <= E cannot be within it of any other segment.  Built by plan_slabs (host).
struct SlabView {
    const uint16_t* p;
    uint32_t ns;
    __device__ __forceinline__ uint32_t cbeg(uint32_t s) const { return p[s]; }
    __device__ __forceinline__ uint32_t dbeg(uint32_t s) const { return p[ns + 1 + s]; }
    __device__ __forceinline__ uint32_t id(uint32_t k) const { return p[2 * (ns + 1) + k]; }
};

__host__ __device__ __forceinline__ uint32_t slab_of(double y, double sy0, double sinv, uint32_t ns) {
    const double f = (y - sy0) * sinv;
    if (!(f >= 0.0)) return 0;  // also NaN
    if (f >= (double)ns) return ns - 1;
    return (uint32_t)f;
}

// Sign of x1*y2 - y1*x2 for exact inputs: the rounded determinant decides when it clears
// the forward error bound 2^-51.4 * (|x1*y2| + |y1*x2|) (plus an absolute term for underflow);
// otherwise exact_det_sign.  Same result as RobustDeterminant.signOfDet2x2.
__device__ __forceinline__ int det_sign(double x1, double y1, double x2, double y2) {
    const double dl = x1 * y2, dr = y1 * x2;
    const double det = dl - dr;
    const double eb = 3.3306690738754716e-16 * (__builtin_fabs(dl) + __builtin_fabs(dr)) + 0x1.0p-1020;
    if (det > eb) return 1;
    if (det < -eb) return -1;
    return exact_det_sign(x1, y1, x2, y2);
}

// One segment of RayCrossingCounter.countSegment(p1, p2) for point p.
__device__ __forceinline__ void count_segment(double px, double py, double p1x, double p1y, double p2x, double p2y,
                                              bool& boundary, int& crossings) {
    const bool live = !(p1x < px && p2x < px);
    const bool at_p2 = px == p2x && py == p2y;
    const bool horiz = p1y == py && p2y == py;
    const bool on_h = horiz && px >= __builtin_fmin(p1x, p2x) && px <= __builtin_fmax(p1x, p2x);
    const bool strad = (p1y > py && p2y <= py) || (p2y > py && p1y <= py);
    if (live && !at_p2 && strad) {
        const double x1 = p1x - px, y1 = p1y - py, x2 = p2x - px, y2 = p2y - py;
        int sg = det_sign(x1, y1, x2, y2);
        boundary = boundary || sg == 0;
        if (y2 < y1) sg = -sg;
        crossings += sg > 0 ? 1 : 0;
    }
    boundary = boundary || (live && (at_p2 || on_h));
}

}  // namespace geohip
