// maskraster.hip - COCO segmentations (polygons, RLE) -> the mask head's grid targets on gfx950 (K18, include/bdetr.h).
//
// One workgroup per object.  Everything is integer until the last line: the numerator N[i,j] = sum over set source pixels of
// OY(y,i) * OX(x,j) is accumulated in LDS with 64-bit integer adds (associative: two calls are bit-identical, whatever the order
// the lanes arrive in), and the target is ONE IEEE fp64 division N / (H h W w) rounded to fp32.  Compiled with -ffp-contract=off
// like detmetric.hip / maskmetric.hip so that the division stays a division.
//
// Geometry.  In units of 1 / (G new_h) of a placed source pixel the source row y covers [base_y + y gn_y, base_y + (y+1) gn_y)
// with base_y = G h off_h, gn_y = G new_h, and the grid row i covers [i c_y, (i+1) c_y) with c_y = H h.  Source rows are
// contiguous, so the rows ys..ye-1 TOGETHER cover one interval and sum over them of OY(y,i) is that interval's overlap with the
// cell: every sum over a run of pixels below is a closed form, never a loop over pixels.  Columns likewise.
//
// Polygons: a band of source rows lives in LDS as a row-major bitmask.  Per ring, lanes over (edge, row) toggle the first pixel
// whose centre is at or right of the crossing; a parity prefix over the row turns toggles into the even-odd fill; the fill is
// ORed into the band's union.  Then lanes over (row, j) take popcounts of the union between the pixels that straddle the cell's
// two sides.  RLE: lanes over one-runs; a column-major run is at most three rectangles (head column, full columns, tail column).
#include "common.h"
#include <limits.h>

namespace {

constexpr int MR_THREADS = 256;
constexpr int MR_MAX_G = 32;             // grid cells per side
constexpr int MR_MAX_DIM = 4096;         // source and canvas extents
constexpr int MR_COORD = 1 << 23;        // |snapped coordinate| (1/256 pixel)
constexpr int MR_BAND_WORDS = 3072;      // 64-bit words per LDS band buffer (two buffers: 48 KiB)
constexpr int MR_KIND_POLY = 1, MR_KIND_RLE = 2;      // 0 = none

typedef unsigned long long u64;

struct mr_geom {
    long long base_y, gn_y, c_y, base_x, gn_x, c_x;
    int G;
};

__device__ __forceinline__ long long ceil_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b > 0) ? q + 1 : q;
}
__device__ __forceinline__ int clamp_coord(int v) { return min(max(v, -MR_COORD), MR_COORD); }

// source rows [ys, ye) x source columns [xs, xe), all set: add the rectangle's overlap with every cell it touches
__device__ void add_rect(u64* s_N, const mr_geom& g, int xs, int xe, int ys, int ye) {
    const long long y0 = g.base_y + ys * g.gn_y, y1 = g.base_y + ye * g.gn_y;
    const long long x0 = g.base_x + xs * g.gn_x, x1 = g.base_x + xe * g.gn_x;
    const int i0 = (int)(y0 / g.c_y), i1 = min((int)((y1 - 1) / g.c_y), g.G - 1);
    const int j0 = (int)(x0 / g.c_x), j1 = min((int)((x1 - 1) / g.c_x), g.G - 1);
    for (int i = i0; i <= i1; ++i) {
        const long long oy = min(y1, (i + 1) * g.c_y) - max(y0, i * g.c_y);
        for (int j = j0; j <= j1; ++j) {
            const long long ox = min(x1, (j + 1) * g.c_x) - max(x0, j * g.c_x);
            atomicAdd(&s_N[i * g.G + j], (u64)(oy * ox));
        }
    }
}

// set bits of the row in [a, b), a < b
__device__ __forceinline__ int pop_range(const u64* row, int a, int b) {
    const int wa = a >> 6, wb = (b - 1) >> 6;
    const u64 ma = ~0ull << (a & 63), mb = ~0ull >> (63 - ((b - 1) & 63));
    if (wa == wb) return __popcll(row[wa] & ma & mb);
    int c = __popcll(row[wa] & ma) + __popcll(row[wb] & mb);
    for (int k = wa + 1; k < wb; ++k) c += __popcll(row[k]);
    return c;
}

__global__ __launch_bounds__(MR_THREADS) void mask_targets_kernel(const int32_t* __restrict__ items, long long n_items,
                                                                  const int32_t* __restrict__ item_off, const int32_t* __restrict__ kind,
                                                                  const int32_t* __restrict__ hw, const int32_t* __restrict__ placement,
                                                                  int M, int G, float* __restrict__ masks, int32_t* __restrict__ area) {
    __shared__ u64 s_N[MR_MAX_G * MR_MAX_G];
    __shared__ u64 s_tog[MR_BAND_WORDS];
    __shared__ u64 s_uni[MR_BAND_WORDS];
    __shared__ int s_xa[MR_MAX_G], s_xb[MR_MAX_G], s_oxa[MR_MAX_G], s_oxb[MR_MAX_G];
    __shared__ int s_area, s_ymin, s_ymax;

    const int o = blockIdx.x, b = o / M, tid = threadIdx.x;
    const int GG = G * G;
    for (int k = tid; k < GG; k += MR_THREADS) s_N[k] = 0ull;
    if (tid == 0) {
        s_area = 0;
        s_ymin = INT_MAX;
        s_ymax = INT_MIN;
    }

    // everything below is uniform over the workgroup: every lane reads the same descriptors
    const int kd = kind[o], h = hw[2 * o], w = hw[2 * o + 1];
    const int32_t* pl = placement + 6 * b;
    const int H = pl[0], W = pl[1], nh = pl[2], nw = pl[3], oh = pl[4], ow = pl[5];
    const long long off0 = item_off[o], off1 = item_off[o + 1];
    bool ok = (kd == MR_KIND_POLY || kd == MR_KIND_RLE) && h >= 1 && h <= MR_MAX_DIM && w >= 1 && w <= MR_MAX_DIM;
    ok = ok && H >= 1 && H <= MR_MAX_DIM && W >= 1 && W <= MR_MAX_DIM && nh >= 1 && nw >= 1 && oh >= 0 && ow >= 0 &&
         (long long)oh + nh <= H && (long long)ow + nw <= W;
    ok = ok && off0 >= 0 && off0 <= off1 && off1 <= n_items;
    mr_geom g;
    g.G = G;
    g.base_y = (long long)G * h * oh;
    g.gn_y = (long long)G * nh;
    g.c_y = (long long)H * h;
    g.base_x = (long long)G * w * ow;
    g.gn_x = (long long)G * nw;
    g.c_x = (long long)W * w;
    const long long D = ok ? g.c_y * g.c_x : 1;
    const int32_t* it = items + off0;
    const long long n = off1 - off0;
    __syncthreads();

    if (ok && kd == MR_KIND_RLE) {
        // items: (start, length) of the one-runs in column-major pixel order
        const long long hwpix = (long long)h * w;
        int my_area = 0;
        for (long long r = tid; r < n / 2; r += MR_THREADS) {
            long long s = it[2 * r], e = s + (long long)it[2 * r + 1];
            s = max(s, 0ll);
            e = min(e, hwpix);
            if (e <= s) continue;
            my_area += (int)(e - s);
            const int x0 = (int)(s / h), y0 = (int)(s % h), x1 = (int)((e - 1) / h), y1 = (int)((e - 1) % h) + 1;
            if (x0 == x1) {
                add_rect(s_N, g, x0, x0 + 1, y0, y1);
            } else {
                add_rect(s_N, g, x0, x0 + 1, y0, h);
                if (x1 > x0 + 1) add_rect(s_N, g, x0 + 1, x1, 0, h);
                add_rect(s_N, g, x1, x1 + 1, 0, y1);
            }
        }
        if (my_area) atomicAdd(&s_area, my_area);
    } else if (ok && kd == MR_KIND_POLY && n >= 2) {
        // items: R, ring offsets e[0..R] in vertices (e[0] = 0, e[R] = V), then V snapped (x, y) pairs
        const long long R = it[0];
        long long V = 0;
        bool pok = R >= 0 && R + 2 <= n;
        if (pok) {
            V = it[1 + R];
            pok = V >= 0 && 2 + R + 2 * V <= n;
        }
        if (pok && R > 0 && V > 0) {
            const int32_t* ring = it + 1;
            const int32_t* vert = it + 2 + R;
            for (long long v = tid; v < V; v += MR_THREADS) {
                const int y = clamp_coord(vert[2 * v + 1]);
                atomicMin(&s_ymin, y);
                atomicMax(&s_ymax, y);
            }
            // per grid column j: the source pixels that straddle the cell's left and right side, and their share of it
            if (tid < G) {
                const long long lo = tid * g.c_x - g.base_x, hi = lo + g.c_x;       // the cell, relative to source column 0
                int xa = lo <= 0 ? 0 : (int)min(lo / g.gn_x, (long long)w);
                int xb = hi <= 0 ? -1 : (int)min((hi - 1) / g.gn_x, (long long)w - 1);
                int oxa = 0, oxb = 0;
                if (xa <= xb) {
                    oxa = (int)(min((xa + 1) * g.gn_x, hi) - max(xa * g.gn_x, lo));
                    oxb = (int)(min((xb + 1) * g.gn_x, hi) - max(xb * g.gn_x, lo));
                }
                s_xa[tid] = xa;
                s_xb[tid] = xb;
                s_oxa[tid] = oxa;
                s_oxb[tid] = oxb;
            }
            __syncthreads();
            // rows whose centre 256 y + 128 lies in [ymin, ymax): no other row is crossed by any edge
            const int row_lo = max(0, (int)ceil_div((long long)s_ymin - 128, 256));
            const int row_hi = min(h - 1, (int)ceil_div((long long)s_ymax - 128, 256) - 1);
            const int wpr = (w + 63) >> 6;
            const int band = MR_BAND_WORDS / wpr;                                   // >= 48 rows
            const u64 tail = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;
            int my_area = 0;
            for (int yb0 = row_lo; yb0 <= row_hi; yb0 += band) {
                const int rows = min(band, row_hi - yb0 + 1);
                for (int k = tid; k < rows * wpr; k += MR_THREADS) {
                    s_tog[k] = 0ull;
                    s_uni[k] = 0ull;
                }
                __syncthreads();
                for (long long r = 0; r < R; ++r) {
                    const long long va = min(max((long long)ring[r], 0ll), V), vb = min(max((long long)ring[r + 1], 0ll), V);
                    const int nv = (int)(vb - va);
                    if (nv < 3) continue;                                           // uniform
                    const int32_t* rv = vert + 2 * va;
                    const int sub = tid & 3;
                    for (int e = tid >> 2; e < nv; e += MR_THREADS / 4) {
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
                            if (x < w) atomicXor(&s_tog[(y - yb0) * wpr + (int)(x >> 6)], 1ull << (x & 63));
                        }
                    }
                    __syncthreads();
                    // parity prefix along each row: toggles -> fill; OR into the union; clear the toggles for the next ring
                    for (int rr = tid; rr < rows; rr += MR_THREADS) {
                        u64 carry = 0ull;
                        for (int k = 0; k < wpr; ++k) {
                            u64 t = s_tog[rr * wpr + k];
                            t ^= t << 1;
                            t ^= t << 2;
                            t ^= t << 4;
                            t ^= t << 8;
                            t ^= t << 16;
                            t ^= t << 32;
                            t ^= carry;
                            carry = (t >> 63) ? ~0ull : 0ull;
                            if (k == wpr - 1) t &= tail;
                            s_uni[rr * wpr + k] |= t;
                            s_tog[rr * wpr + k] = 0ull;
                        }
                    }
                    __syncthreads();
                }
                // accumulate: lanes over (row, grid column)
                for (int k = tid; k < rows * wpr; k += MR_THREADS) my_area += __popcll(s_uni[k]);
                for (int item = tid; item < rows * G; item += MR_THREADS) {
                    const int rr = item / G, j = item - rr * G;
                    const int xa = s_xa[j], xb = s_xb[j];
                    if (xa > xb) continue;
                    const u64* row = s_uni + rr * wpr;
                    long long Rj = (long long)((row[xa >> 6] >> (xa & 63)) & 1ull) * s_oxa[j];
                    if (xb > xa) {
                        Rj += (long long)((row[xb >> 6] >> (xb & 63)) & 1ull) * s_oxb[j];
                        if (xb > xa + 1) Rj += g.gn_x * pop_range(row, xa + 1, xb);
                    }
                    if (Rj == 0) continue;
                    const int y = yb0 + rr;
                    const long long y0 = g.base_y + y * g.gn_y, y1 = y0 + g.gn_y;
                    const int i0 = (int)(y0 / g.c_y), i1 = min((int)((y1 - 1) / g.c_y), G - 1);
                    for (int i = i0; i <= i1; ++i) {
                        const long long oy = min(y1, (i + 1) * g.c_y) - max(y0, i * g.c_y);
                        atomicAdd(&s_N[i * G + j], (u64)(oy * Rj));
                    }
                }
                __syncthreads();
            }
            if (my_area) atomicAdd(&s_area, my_area);
        }
    }
    __syncthreads();
    float* out = masks + (long long)o * GG;
    for (int k = tid; k < GG; k += MR_THREADS) out[k] = (float)((double)(long long)s_N[k] / (double)D);
    if (tid == 0) area[o] = s_area;
}

}  // namespace

extern "C" int bdetr_mask_targets(const int32_t* items, int64_t n_items, const int32_t* item_off, const int32_t* kind, const int32_t* hw,
                                  const int32_t* placement, int B, int M, int G, float* masks, int32_t* area, void* stream) {
    BDETR_CHECK_ARG(item_off && kind && hw && placement && masks && area && (items || n_items == 0),
                    "bdetr_mask_targets: null pointer (only items may be null, with n_items = 0)");
    BDETR_CHECK_ARG(B > 0 && M > 0 && (int64_t)B * M <= (1 << 24) && G >= 1 && G <= MR_MAX_G && n_items >= 0 && n_items <= INT32_MAX,
                    "bdetr_mask_targets: bad sizes B=%d M=%d G=%d n_items=%lld (limits: B, M >= 1, B M <= 2^24, G in [1, %d], n_items in [0, 2^31))",
                    B, M, G, (long long)n_items, MR_MAX_G);
    hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)(B * M)), dim3(MR_THREADS), 0, (hipStream_t)stream, items, (long long)n_items,
                       item_off, kind, hw, placement, M, G, masks, area);
    return bdetr_launch_status("mask_targets");
}
