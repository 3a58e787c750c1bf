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
// Polygons: mask_scan.h fills a band of source rows in LDS (the source-mask rule, shared with maskimage.hip's K20); then lanes
// over (row, j) take popcounts of the band's union between the pixels that straddle the cell's two sides and the band is dropped.
// RLE: lanes over one-runs; a column-major run is at most three rectangles (head column, full columns, tail column).
#include "mask_scan.h"

using namespace maskscan;

namespace {

constexpr int MR_MAX_G = 32;             // grid cells per side

struct mr_geom {
    long long base_y, gn_y, c_y, base_x, gn_x, c_x;
    int G;
};

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

__global__ __launch_bounds__(SCAN_THREADS) void mask_targets_kernel(const int32_t* __restrict__ items, long long n_items,
                                                                    const int32_t* __restrict__ item_off, const int32_t* __restrict__ kind,
                                                                    const int32_t* __restrict__ hw, const int32_t* __restrict__ placement,
                                                                    int M, int G, float* __restrict__ masks, int32_t* __restrict__ area) {
    __shared__ u64 s_N[MR_MAX_G * MR_MAX_G];
    __shared__ scan_lds s_scan;
    __shared__ int s_xa[MR_MAX_G], s_xb[MR_MAX_G], s_oxa[MR_MAX_G], s_oxb[MR_MAX_G];
    __shared__ int s_area;

    const int o = blockIdx.x, b = o / M, tid = threadIdx.x;
    const int GG = G * G;
    for (int k = tid; k < GG; k += SCAN_THREADS) s_N[k] = 0ull;
    if (tid == 0) {
        s_area = 0;
        s_scan.reset();
    }

    // everything below is uniform over the workgroup: every lane reads the same descriptors
    const segment sg = load_segment(items, n_items, item_off, kind, hw, o);
    const int h = sg.h, w = sg.w;
    const int32_t* pl = placement + 6 * b;
    const int H = pl[0], W = pl[1], nh = pl[2], nw = pl[3], oh = pl[4], ow = pl[5];
    const bool ok = sg.ok && H >= 1 && H <= MAX_DIM && W >= 1 && W <= MAX_DIM && nh >= 1 && nw >= 1 && oh >= 0 && ow >= 0 &&
                    (long long)oh + nh <= H && (long long)ow + nw <= W;
    mr_geom g;
    g.G = G;
    g.base_y = (long long)G * h * oh;
    g.gn_y = (long long)G * nh;
    g.c_y = (long long)H * h;
    g.base_x = (long long)G * w * ow;
    g.gn_x = (long long)G * nw;
    g.c_x = (long long)W * w;
    const long long D = ok ? g.c_y * g.c_x : 1;
    rings p;
    __syncthreads();

    if (ok && sg.kind == KIND_RLE) {
        // items: (start, length) of the one-runs in column-major pixel order
        const long long hwpix = (long long)h * w;
        int my_area = 0;
        for (long long r = tid; r < sg.n / 2; r += SCAN_THREADS) {
            long long s = sg.it[2 * r], e = s + (long long)sg.it[2 * r + 1];
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
    } else if (ok && sg.kind == KIND_POLY && parse_rings(sg, p)) {
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
        int row_lo, row_hi;
        row_range(s_scan, p, h, row_lo, row_hi);                                // synchronises: the column table is visible after it
        const int wpr = (w + 63) >> 6;
        const int band = BAND_WORDS / wpr;                                      // >= 48 rows
        const u64* s_uni = s_scan.uni;
        int my_area = 0;
        for (int yb0 = row_lo; yb0 <= row_hi; yb0 += band) {
            const int rows = min(band, row_hi - yb0 + 1);
            clear_band(s_scan, rows * wpr);
            fill_rings(s_scan, p, w, yb0, rows);
            // accumulate: lanes over (row, grid column)
            for (int k = tid; k < rows * wpr; k += SCAN_THREADS) my_area += __popcll(s_uni[k]);
            for (int item = tid; item < rows * G; item += SCAN_THREADS) {
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
    __syncthreads();
    float* out = masks + (long long)o * GG;
    for (int k = tid; k < GG; k += SCAN_THREADS) out[k] = (float)((double)(long long)s_N[k] / (double)D);
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
    hipLaunchKernelGGL(mask_targets_kernel, dim3((unsigned)(B * M)), dim3(SCAN_THREADS), 0, (hipStream_t)stream, items, (long long)n_items,
                       item_off, kind, hw, placement, M, G, masks, area);
    return bdetr_launch_status("mask_targets");
}
