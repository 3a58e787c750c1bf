// maskimage.hip - mask AP at image resolution on gfx950 (K19-K22, include/bdetr.h): the query masks upsampled to the image
// (bilinear on the logits, cut at 0), the ground truths' exact source bitmasks, the popcount intersection of the two, and COCOeval's
// matching fed from that intersection.  evaluation.CocoImageMaskEvaluator chains the four.  Three rules are shared and live in
// headers: the pixel's value (mask_upsample.h, with panopticmerge.hip), the source mask (mask_scan.h, with maskraster.hip) and the
// matcher (coco_match.h, with detmetric.hip and maskmetric.hip; K22 is its instantiation on the intersection, inter_iou).
//
// One layout for every mask of a batch: uint64 [Hm, Wm], Hm = max height, Wm = ceil(max width / 64), pixel (x, y) is bit x mod 64 of
// word [y, x div 64]; bits at x >= w_b and rows y >= h_b are zero and are WRITTEN as zero by K19 and K20 (no memset is relied on).
//
// Compiled with -ffp-contract=off like maskmetric.hip; the two headers whose arithmetic depends on it say so themselves.
#include "coco_match.h"
#include "mask_scan.h"
#include "mask_upsample.h"

using namespace cocomatch;
using namespace maskscan;
using namespace maskup;

namespace {

constexpr int MI_THREADS = SCAN_THREADS;

// ---------------------------------------------------------------------------------------------------------------------
// K19: logits [B,N,G,G] -> bits [B,N,Hm,Wm], pop [B,N]
// ---------------------------------------------------------------------------------------------------------------------
// One workgroup per (image, query).  LDS (dynamic): the x axis' weights double [64 Wm] and cell pairs int [64 Wm] (ia | ib << 8),
// then the G x G logits.  A wave owns runs of 64 consecutive output words; per word, lane l evaluates pixel x = 64 wd + l and the
// wave's ballot IS the word; lane k keeps word k of the run and the run is stored with one coalesced 512-byte store.  The y axis'
// rule is wave-uniform and is evaluated when the run enters a new row.
__global__ __launch_bounds__(MI_THREADS) void mask_upsample_bits_kernel(const float* __restrict__ logits, const int32_t* __restrict__ image_hw,
                                                                        int N, int G, int Hm, int Wm, u64* __restrict__ bits,
                                                                        int32_t* __restrict__ pop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_pop;
    const int Wx = Wm * 64, GG = G * G;
    double* s_tx = reinterpret_cast<double*>(smem);
    int* s_ix = reinterpret_cast<int*>(s_tx + Wx);
    float* s_L = reinterpret_cast<float*>(s_ix + Wx);

    const int o = blockIdx.x, b = o / N, tid = threadIdx.x;
    const int h = min(max(image_hw[2 * b], 0), Hm), w = min(max(image_hw[2 * b + 1], 0), Wx);      // never past the buffers
    const float* L = logits + (int64_t)o * GG;
    for (int k = tid; k < GG; k += MI_THREADS) s_L[k] = L[k];
    for (int x = tid; x < w; x += MI_THREADS) {
        const axis a = axis_rule(x, w, G);
        s_tx[x] = a.t;
        s_ix[x] = a.ia | (a.ib << 8);
    }
    if (tid == 0) s_pop = 0;
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int total = Hm * Wm;                                   // <= 4096 * 64
    u64* out = bits + (int64_t)o * total;
    int my_pop = 0;                                              // wave-uniform
    for (int first = wave * 64; first < total; first += MI_THREADS) {
        const int cnt = min(64, total - first);
        int y = first / Wm, wd = first - y * Wm;
        int cur_y = -1;
        const float *r0 = s_L, *r1 = s_L;
        double ty = 0.0, uy = 1.0;
        u64 mine = 0ull;
        for (int k = 0; k < cnt; ++k) {                          // everything but `on` is wave-uniform: every lane reaches the ballot
            u64 word = 0ull;
            if (y < h && wd * 64 < w) {
                if (y != cur_y) {
                    const axis a = axis_rule(y, h, G);
                    r0 = s_L + a.ia * G;
                    r1 = s_L + a.ib * G;
                    ty = a.t;
                    uy = 1.0 - ty;
                    cur_y = y;
                }
                const int x = wd * 64 + lane;
                bool on = false;
                if (x < w) {
                    const int ix = s_ix[x], xa = ix & 255, xb = ix >> 8;
                    const double tx = s_tx[x], ux = 1.0 - tx;
                    on = bilinear(ux, tx, uy, ty, r0[xa], r0[xb], r1[xa], r1[xb]) > 0.0;      // NaN > 0 is false
                }
                word = __ballot(on);
                my_pop += __popcll(word);
            }
            if (k == lane) mine = word;
            if (++wd == Wm) {
                wd = 0;
                ++y;
            }
        }
        if (lane < cnt) out[first + lane] = mine;
    }
    if (lane == 0 && my_pop) atomicAdd(&s_pop, my_pop);
    __syncthreads();
    if (tid == 0) pop[o] = s_pop;
}

// ---------------------------------------------------------------------------------------------------------------------
// K20: the segments pack -> bits [B,M,Hm,Wm], pop [B,M].  The source mask is mask_scan.h's (K18's rule): maskraster.hip folds
// each band into grid cells and drops it, here it is stored.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MI_THREADS) void mask_source_bits_kernel(const int32_t* __restrict__ items, long long n_items,
                                                                      const int32_t* __restrict__ item_off, const int32_t* __restrict__ kind,
                                                                      const int32_t* __restrict__ hw, int Hm, int Wm, u64* __restrict__ bits,
                                                                      int32_t* __restrict__ pop) {
    __shared__ scan_lds s_scan;
    __shared__ int s_area;

    const int o = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_area = 0;
        s_scan.reset();
    }
    // everything below is uniform over the workgroup: every lane reads the same descriptors
    const segment sg = load_segment(items, n_items, item_off, kind, hw, o);
    const int h = sg.h, w = sg.w;
    const bool ok = sg.ok && h <= Hm && ((w + 63) >> 6) <= Wm;
    const int total = Hm * Wm;
    u64* out = bits + (int64_t)o * total;
    __syncthreads();

    // the rows that can hold a set bit: [row_lo, row_hi]
    int row_lo = 0, row_hi = -1;
    rings p;
    if (ok && sg.kind == KIND_RLE) row_hi = h - 1;
    else if (ok && sg.kind == KIND_POLY && parse_rings(sg, p)) row_range(s_scan, p, h, row_lo, row_hi);      // synchronises
    if (row_hi < row_lo) {
        row_lo = 0;
        row_hi = -1;
    }
    for (int k = tid; k < row_lo * Wm; k += MI_THREADS) out[k] = 0ull;
    for (int k = (row_hi + 1) * Wm + tid; k < total; k += MI_THREADS) out[k] = 0ull;

    if (row_hi >= row_lo) {
        const int wpr = (w + 63) >> 6;
        const int band = BAND_WORDS / wpr;                                          // >= 48 rows
        u64* s_uni = s_scan.uni;
        int my_area = 0;
        for (int yb0 = row_lo; yb0 <= row_hi; yb0 += band) {
            const int rows = min(band, row_hi - yb0 + 1);
            clear_band(s_scan, rows * wpr);
            if (sg.kind == KIND_RLE) {
                // items: (start, length) of the one-runs in column-major pixel order.  16 lanes per run: per column of the run,
                // the lanes set the run's rows inside the band
                const int hwpix = h * w;                                            // <= 2^24
                const int sub = tid & 15;
                for (long long r = tid >> 4; r < sg.n / 2; r += MI_THREADS / 16) {
                    long long s = sg.it[2 * r], e = s + (long long)sg.it[2 * r + 1];
                    s = max(s, 0ll);
                    e = min(e, (long long)hwpix);
                    if (e <= s) continue;
                    const int x0 = (int)(s / h), y0 = (int)(s % h), x1 = (int)((e - 1) / h), y1 = (int)((e - 1) % h) + 1;
                    for (int x = x0; x <= x1; ++x) {
                        const int ya = max(x == x0 ? y0 : 0, yb0), ye = min(x == x1 ? y1 : h, yb0 + rows);
                        for (int y = ya + sub; y < ye; y += 16) atomicOr(&s_uni[(y - yb0) * wpr + (x >> 6)], 1ull << (x & 63));
                    }
                }
                __syncthreads();
            } else {
                fill_rings(s_scan, p, w, yb0, rows);
            }
            // store the band: its rows in full, the words past the image's own with zeros
            u64* orow = out + (int64_t)yb0 * Wm;
            for (int k = tid; k < rows * Wm; k += MI_THREADS) {
                const int rr = k / Wm, wd = k - rr * Wm;
                const u64 v = wd < wpr ? s_uni[rr * wpr + wd] : 0ull;
                my_area += __popcll(v);
                orow[k] = v;
            }
            __syncthreads();
        }
        if (my_area) atomicAdd(&s_area, my_area);
    }
    __syncthreads();
    if (tid == 0) pop[o] = s_area;
}

// ---------------------------------------------------------------------------------------------------------------------
// K21: inter[b,n,m] = sum over words of popcount(det[b,n] & gt[b,m]) for m < num_objects[b]
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MI_TILE = 8;                // detections x ground truths per workgroup: 64 counters per lane
constexpr int MI_SPLIT_CHUNKS = 1024;     // loads per mask a workgroup streams at least (x 256 lanes: 4 per lane)
constexpr int MI_MAX_SPLITS = 64;

template <int VEC>
struct mi_words;
template <>
struct mi_words<1> {
    u64 x;
    __device__ __forceinline__ void load(const u64* p, int64_t c) { x = p[c]; }
    __device__ __forceinline__ int both(const mi_words& g) const { return __popcll(x & g.x); }
};
template <>
struct mi_words<2> {
    ulonglong2 v;
    __device__ __forceinline__ void load(const u64* p, int64_t c) { v = reinterpret_cast<const ulonglong2*>(p)[c]; }      // 16 bytes
    __device__ __forceinline__ int both(const mi_words& g) const { return __popcll(v.x & g.v.x) + __popcll(v.y & g.v.y); }
};

// Grid (tiles of 8 detections x tiles of 8 ground truths, word splits, B).  A lane streams its share of the words of all 16 masks
// (one load of VEC words each per step) and keeps the 8 x 8 popcounts in registers: a detection mask is read once per 8 ground
// truths instead of once per ground truth, and the ground truths' re-reads (once per 8 detections) come from L2.  Tiles at or past
// num_objects leave at once.  The 64 counters are summed over the wave by a transposing butterfly (63 shuffles: each step halves
// the counters a lane still carries, lane a ends with counter a), and each wave adds its sums with integer atomics: associative,
// so two calls give the same bits.  Rows past N / M are clamped for the loads and dropped at the end.
template <int VEC>
__global__ __launch_bounds__(MI_THREADS) void mask_inter_kernel(const u64* __restrict__ det, const u64* __restrict__ gt,
                                                                const int32_t* __restrict__ num_objects, int N, int M, int64_t words,
                                                                int tiles_m, int64_t split_chunks, int32_t* __restrict__ inter) {
    const int b = blockIdx.z, tn = blockIdx.x / tiles_m, tm = blockIdx.x - tn * tiles_m;
    const int n_obj = max(0, min(num_objects[b], M));
    const int n0 = tn * MI_TILE, m0 = tm * MI_TILE;
    if (m0 >= n_obj) return;                                     // uniform
    const int64_t chunks = words / VEC;
    const int64_t c0 = (int64_t)blockIdx.y * split_chunks, c1 = min(chunks, c0 + split_chunks);
    const u64* dp[MI_TILE];
    const u64* gp[MI_TILE];
#pragma unroll
    for (int i = 0; i < MI_TILE; ++i) {
        dp[i] = det + ((int64_t)b * N + min(n0 + i, N - 1)) * words;
        gp[i] = gt + ((int64_t)b * M + min(m0 + i, M - 1)) * words;
    }
    int acc[MI_TILE * MI_TILE];
#pragma unroll
    for (int k = 0; k < MI_TILE * MI_TILE; ++k) acc[k] = 0;
    for (int64_t c = c0 + threadIdx.x; c < c1; c += MI_THREADS) {
        mi_words<VEC> d[MI_TILE], g[MI_TILE];
#pragma unroll
        for (int i = 0; i < MI_TILE; ++i) {
            d[i].load(dp[i], c);
            g[i].load(gp[i], c);
        }
#pragma unroll
        for (int i = 0; i < MI_TILE; ++i)
#pragma unroll
            for (int j = 0; j < MI_TILE; ++j) acc[i * MI_TILE + j] += d[i].both(g[j]);
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int o = 32 >> s;                                   // lanes o apart pair up; `o` counters stay per lane
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int k = 0; k < o; ++k) {
            const int send = up ? acc[k] : acc[k + o];
            const int keep = up ? acc[k + o] : acc[k];
            acc[k] = keep + __shfl_xor(send, o, 64);
        }
    }
    const int i = lane >> 3, j = lane & 7;                       // lane a carries counter a = 8 i + j
    if (n0 + i < N && m0 + j < n_obj && acc[0]) atomicAdd(&inter[((int64_t)b * N + n0 + i) * M + m0 + j], acc[0]);
}

bool mask_layout_ok(int Hm, int Wm) { return Hm >= 1 && Hm <= MAX_DIM && Wm >= 1 && Wm <= MAX_DIM / 64; }

}  // namespace

extern "C" int bdetr_mask_upsample_bits(const float* logits, const int32_t* image_hw, int B, int N, int G, int Hm, int Wm, uint64_t* bits,
                                        int32_t* pop, void* stream) {
    BDETR_CHECK_ARG(logits && image_hw && bits && pop, "bdetr_mask_upsample_bits: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && (int64_t)B * N <= (1 << 24) && G >= 1 && G <= MAX_G && mask_layout_ok(Hm, Wm),
                    "bdetr_mask_upsample_bits: bad sizes B=%d N=%d G=%d Hm=%d Wm=%d (limits: B, N >= 1, B N <= 2^24, G in [1, %d], Hm in [1, %d], "
                    "Wm in [1, %d])", B, N, G, Hm, Wm, MAX_G, MAX_DIM, MAX_DIM / 64);
    const size_t lds = (size_t)Wm * 64 * 12 + (size_t)G * G * 4;      // at most 52 KiB
    hipLaunchKernelGGL(mask_upsample_bits_kernel, dim3((unsigned)(B * N)), dim3(MI_THREADS), lds, (hipStream_t)stream, logits, image_hw, N, G,
                       Hm, Wm, reinterpret_cast<u64*>(bits), pop);
    return bdetr_launch_status("mask_upsample_bits");
}

extern "C" int bdetr_mask_source_bits(const int32_t* items, int64_t n_items, const int32_t* item_off, const int32_t* kind, const int32_t* hw,
                                      int B, int M, int Hm, int Wm, uint64_t* bits, int32_t* pop, void* stream) {
    BDETR_CHECK_ARG(item_off && kind && hw && bits && pop && (items || n_items == 0),
                    "bdetr_mask_source_bits: null pointer (only items may be null, with n_items = 0)");
    BDETR_CHECK_ARG(B > 0 && M > 0 && (int64_t)B * M <= (1 << 24) && n_items >= 0 && n_items <= INT32_MAX && mask_layout_ok(Hm, Wm),
                    "bdetr_mask_source_bits: bad sizes B=%d M=%d Hm=%d Wm=%d n_items=%lld (limits: B, M >= 1, B M <= 2^24, Hm in [1, %d], "
                    "Wm in [1, %d], n_items in [0, 2^31))", B, M, Hm, Wm, (long long)n_items, MAX_DIM, MAX_DIM / 64);
    hipLaunchKernelGGL(mask_source_bits_kernel, dim3((unsigned)(B * M)), dim3(MI_THREADS), 0, (hipStream_t)stream, items, (long long)n_items,
                       item_off, kind, hw, Hm, Wm, reinterpret_cast<u64*>(bits), pop);
    return bdetr_launch_status("mask_source_bits");
}

extern "C" int bdetr_mask_inter(const uint64_t* det_bits, const uint64_t* gt_bits, const int32_t* num_objects, int B, int N, int M, int Hm,
                                int Wm, int32_t* inter, void* stream) {
    BDETR_CHECK_ARG(det_bits && gt_bits && num_objects && inter, "bdetr_mask_inter: null pointer");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && mask_layout_ok(Hm, Wm),
                    "bdetr_mask_inter: bad sizes B=%d N=%d M=%d Hm=%d Wm=%d (limits: B in [1, 65535], N in [1, %d], M in [1, %d], Hm in [1, %d], "
                    "Wm in [1, %d])", B, N, M, Hm, Wm, MAX_N, MAX_M, MAX_DIM, MAX_DIM / 64);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bdetr_zero_bytes(inter, (size_t)B * N * M * sizeof(int32_t), st)) return e;      // the waves ADD into it
    const int64_t words = (int64_t)Hm * Wm;
    // 16-byte loads need an even word count per mask and 16-byte aligned bases; otherwise one word per load
    const bool wide = words % 2 == 0 && ((uintptr_t)det_bits % 16 == 0) && ((uintptr_t)gt_bits % 16 == 0);
    const int64_t chunks = wide ? words / 2 : words;
    int64_t splits = cdiv64(chunks, MI_SPLIT_CHUNKS);
    if (splits > MI_MAX_SPLITS) splits = MI_MAX_SPLITS;
    const int64_t split_chunks = cdiv64(chunks, splits);
    const int tiles_n = (N + MI_TILE - 1) / MI_TILE, tiles_m = (M + MI_TILE - 1) / MI_TILE;
    const dim3 grid((unsigned)(tiles_n * tiles_m), (unsigned)splits, (unsigned)B);
    const u64* d = reinterpret_cast<const u64*>(det_bits);
    const u64* g = reinterpret_cast<const u64*>(gt_bits);
    if (wide)
        hipLaunchKernelGGL(mask_inter_kernel<2>, grid, dim3(MI_THREADS), 0, st, d, g, num_objects, N, M, words, tiles_m, split_chunks, inter);
    else
        hipLaunchKernelGGL(mask_inter_kernel<1>, grid, dim3(MI_THREADS), 0, st, d, g, num_objects, N, M, words, tiles_m, split_chunks, inter);
    return bdetr_launch_status("mask_inter");
}

extern "C" int bdetr_mask_match_coco_inter(const float* score, const int32_t* label, const int32_t* inter, const int32_t* det_pop,
                                           const int32_t* gt_label, const int32_t* gt_pop, const uint8_t* gt_crowd, const float* gt_area,
                                           const int32_t* num_objects, const int32_t* image_hw, const int32_t* pix, const double* area_ranges,
                                           const double* thresholds, int B, int N, int M, int C, int T, int A, int max_dets, int32_t* order,
                                           int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count,
                                           void* stream) {
    BDETR_CHECK_ARG(score && label && inter && det_pop && gt_label && gt_pop && gt_crowd && num_objects && image_hw && pix && area_ranges &&
                    thresholds && order && class_rank && tp_bits && ig_bits && matched_gt && gt_count,
                    "bdetr_mask_match_coco_inter: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && C >= 3 && C <= MAX_C && T > 0 &&
                    T <= MAX_T && A > 0 && A <= MAX_A && max_dets > 0,
                    "bdetr_mask_match_coco_inter: bad sizes B=%d N=%d M=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, "
                    "C in [3, %d], T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, C, T, A, max_dets, MAX_N, MAX_M, MAX_C,
                    MAX_T, MAX_A);
    const inter_source src = {inter, det_pop, gt_pop, pix};
    const size_t base = carve<inter_iou<false>, true>(N, M, src).total, staged = carve<inter_iou<true>, true>(N, M, src).total;
    BDETR_CHECK_ARG(base <= LDS_LIMIT, "bdetr_mask_match_coco_inter: N=%d M=%d need %zu bytes of LDS per image; the limit is %zu", N, M, base,
                    LDS_LIMIT);
    const match_thresholds thr(thresholds, T);
    if (staged <= LDS_LIMIT)
        hipLaunchKernelGGL((coco_match_kernel<inter_iou<true>, true>), dim3(B, A), dim3(64 * T), staged, (hipStream_t)stream, src, score, label,
                           gt_label, gt_crowd, gt_area, num_objects, image_hw, area_ranges, thr, B, N, M, C, T, max_dets, order, class_rank, tp_bits,
                           ig_bits, matched_gt, gt_count);
    else
        hipLaunchKernelGGL((coco_match_kernel<inter_iou<false>, true>), dim3(B, A), dim3(64 * T), base, (hipStream_t)stream, src, score, label,
                           gt_label, gt_crowd, gt_area, num_objects, image_hw, area_ranges, thr, B, N, M, C, T, max_dets, order, class_rank, tp_bits,
                           ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("mask_match_coco_inter");
}
