// mask_scan.h - the source mask of a COCO segmentation on gfx950 (K18's rule, include/bdetr.h: the project's own, the one place
// where it deliberately differs from pycocotools), written once.  A pixel is inside a polygon when its centre is inside some ring
// by the even-odd rule, on coordinates snapped to 1/256 pixel: integers throughout.  Two kernels use it, one workgroup of
// SCAN_THREADS per object each:
//   maskraster.hip  mask_targets_kernel (K18)      folds every band into the mask head's grid cells and drops it
//   maskimage.hip   mask_source_bits_kernel (K20)  stores every band
// A band of source rows lives in LDS as a row-major bitmask.  Per ring, lanes over (edge, row) toggle the first pixel whose centre
// is at or right of the crossing; a parity prefix over the row turns toggles into the even-odd fill; the fill is ORed into the
// band's union.
//
// Every function here that synchronises says so: it must be reached by the whole workgroup.  Both kernels call them under
// conditions on the object's descriptors only, which every lane reads alike - keep it that way.
#pragma once
#include "common.h"
#include <limits.h>

namespace maskscan {

typedef unsigned long long u64;

constexpr int SCAN_THREADS = 256;
constexpr int MAX_DIM = 4096;            // source, canvas and image extents
constexpr int COORD = 1 << 23;           // |snapped coordinate| (1/256 pixel)
constexpr int BAND_WORDS = 3072;         // 64-bit words per LDS band buffer (two buffers: 48 KiB)
constexpr int KIND_POLY = 1, KIND_RLE = 2;      // 0 = none

__device__ __forceinline__ long long ceil_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b > 0) ? q + 1 : q;
}
__device__ __forceinline__ int clamp_coord(int v) { return min(max(v, -COORD), COORD); }

// the workgroup's static LDS for the scan; thread 0 calls reset() before the kernel's first synchronise
struct scan_lds {
    u64 tog[BAND_WORDS];
    u64 uni[BAND_WORDS];
    int ymin, ymax;
    __device__ __forceinline__ void reset() {
        ymin = INT_MAX;
        ymax = INT_MIN;
    }
};

// object o of the pack: its kind, its source extent and its items.  Uniform over the workgroup.
struct segment {
    int kind, h, w;
    const int32_t* it;
    long long n;
    bool ok;                             // a polygon or an RLE, extents in [1, MAX_DIM], items inside the pack
};
__device__ __forceinline__ segment load_segment(const int32_t* items, long long n_items, const int32_t* item_off, const int32_t* kind,
                                                const int32_t* hw, int o) {
    segment s;
    s.kind = kind[o];
    s.h = hw[2 * o];
    s.w = hw[2 * o + 1];
    const long long off0 = item_off[o], off1 = item_off[o + 1];
    s.ok = (s.kind == KIND_POLY || s.kind == KIND_RLE) && s.h >= 1 && s.h <= MAX_DIM && s.w >= 1 && s.w <= MAX_DIM &&
           off0 >= 0 && off0 <= off1 && off1 <= n_items;
    s.it = items + off0;
    s.n = off1 - off0;
    return s;
}

// a polygon's items: R, ring offsets e[0..R] in vertices (e[0] = 0, e[R] = V), then V snapped (x, y) pairs
struct rings {
    long long R, V;
    const int32_t *ring, *vert;
};
// false: nothing to fill (no ring, no vertex, or counts that do not fit the items)
__device__ __forceinline__ bool parse_rings(const segment& s, rings& p) {
    if (s.n < 2) return false;
    p.R = s.it[0];
    if (!(p.R >= 0 && p.R + 2 <= s.n)) return false;
    p.V = s.it[1 + p.R];
    if (!(p.V >= 0 && 2 + p.R + 2 * p.V <= s.n)) return false;
    p.ring = s.it + 1;
    p.vert = s.it + 2 + p.R;
    return p.R > 0 && p.V > 0;
}

// SYNCHRONISES.  The rows that can hold a set bit, [row_lo, row_hi] (empty: row_hi < row_lo): those whose centre 256 y + 128
// lies in [ymin, ymax) of the vertices - no other row is crossed by any edge.
__device__ __forceinline__ void row_range(scan_lds& s, const rings& p, int h, int& row_lo, int& row_hi) {
    for (long long v = threadIdx.x; v < p.V; v += SCAN_THREADS) {
        const int y = clamp_coord(p.vert[2 * v + 1]);
        atomicMin(&s.ymin, y);
        atomicMax(&s.ymax, y);
    }
    __syncthreads();
    row_lo = max(0, (int)ceil_div((long long)s.ymin - 128, 256));
    row_hi = min(h - 1, (int)ceil_div((long long)s.ymax - 128, 256) - 1);
}

// SYNCHRONISES.  Zero the first `words` words of both band buffers.
__device__ __forceinline__ void clear_band(scan_lds& s, int words) {
    for (int k = threadIdx.x; k < words; k += SCAN_THREADS) {
        s.tog[k] = 0ull;
        s.uni[k] = 0ull;
    }
    __syncthreads();
}

// SYNCHRONISES (twice per ring of three vertices or more).  OR the fill of every ring into s.uni for the band of `rows` source
// rows from yb0, ceil(w / 64) words a row; s.tog must be zero on entry and is zero again on return.
__device__ __forceinline__ void fill_rings(scan_lds& s, const rings& p, int w, int yb0, int rows) {
    const int tid = threadIdx.x, wpr = (w + 63) >> 6;
    const u64 tail = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;
    for (long long r = 0; r < p.R; ++r) {
        const long long va = min(max((long long)p.ring[r], 0ll), p.V), vb = min(max((long long)p.ring[r + 1], 0ll), p.V);
        const int nv = (int)(vb - va);
        if (nv < 3) continue;                                           // uniform
        const int32_t* rv = p.vert + 2 * va;
        const int sub = tid & 3;
        for (int e = tid >> 2; e < nv; e += SCAN_THREADS / 4) {
            const int e2 = e + 1 == nv ? 0 : e + 1;
            int ax = clamp_coord(rv[2 * e]), ay = clamp_coord(rv[2 * e + 1]);
            int bx = clamp_coord(rv[2 * e2]), by = clamp_coord(rv[2 * e2 + 1]);
            if (ay == by) continue;                                     // horizontal edges never cross
            if (ay > by) {
                int t = ax; ax = bx; bx = t;
                t = ay; ay = by; by = t;
            }
            // the edge crosses the rows with lo.y <= cy < hi.y
            const int ya = max(yb0, (int)ceil_div((long long)ay - 128, 256));
            const int ye = min(yb0 + rows - 1, (int)ceil_div((long long)by - 128, 256) - 1);
            const long long dy = (long long)by - ay, dx = (long long)bx - ax;
            for (int y = ya + sub; y <= ye; y += 4) {
                const long long cy = 256ll * y + 128;
                // the crossing counts for cx with (cy - lo.y) dx <= (cx - lo.x) dy: the first such centre
                const long long t = ax + ceil_div((cy - ay) * dx, dy);
                long long x = ceil_div(t - 128, 256);
                if (x < 0) x = 0;
                if (x < w) atomicXor(&s.tog[(y - yb0) * wpr + (int)(x >> 6)], 1ull << (x & 63));
            }
        }
        __syncthreads();
        // parity prefix along each row: toggles -> fill; OR into the union; clear the toggles for the next ring
        for (int rr = tid; rr < rows; rr += SCAN_THREADS) {
            u64 carry = 0ull;
            for (int k = 0; k < wpr; ++k) {
                u64 t = s.tog[rr * wpr + k];
                t ^= t << 1;
                t ^= t << 2;
                t ^= t << 4;
                t ^= t << 8;
                t ^= t << 16;
                t ^= t << 32;
                t ^= carry;
                carry = (t >> 63) ? ~0ull : 0ull;
                if (k == wpr - 1) t &= tail;
                s.uni[rr * wpr + k] |= t;
                s.tog[rr * wpr + k] = 0ull;
            }
        }
        __syncthreads();
    }
}

}  // namespace maskscan
