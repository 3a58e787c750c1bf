// maskmetric.hip - on-GPU mask matching for COCO-style mask AP (pycocotools' iouType="segm") on gfx950: masks are packed into
// 64-bit words (one wave ballot per word), and per image the detections are ranked, truncated per class and matched to the
// ground truths at every IoU threshold exactly as detmetric.hip does for boxes - only the IoU source differs: popcounts of
// packed words instead of box corners.  The host accumulates as for boxes (evaluation.py).
//
// Compiled with -ffp-contract=off, as detmetric.hip is.  The IoU is one IEEE fp64 division of two exact integers, so equal
// rationals (2/4 and 3/6) give equal doubles and 1/2 meets the threshold 0.5: ties and IoUs ON a threshold are the normal case
// with integer pixel counts, and NumPy's count_nonzero ratio is reproduced bit for bit.
#include "common.h"

namespace {

constexpr int MSK_MAX_N = 1024;      // queries per image
constexpr int MSK_MAX_M = 1024;      // ground-truth rows per image (16 matched bits per lane)
constexpr int MSK_MAX_C = 65536;     // classes
constexpr int MSK_MAX_T = 15;        // thresholds: bits 0..14 of tp_bits, bit 15 = keep
constexpr unsigned MSK_KEEP_BIT = 0x8000u;
constexpr size_t MSK_LDS_LIMIT = 64 * 1024;      // the default dynamic LDS of a workgroup (no opt-in to the CU's 160 KiB)

struct mask_thresholds { double v[MSK_MAX_T + 1]; };

// One wave per row.  Lane l of step w holds element 64 w + l (a coalesced 256-byte load); the wave's ballot of the predicate is
// the packed word, lanes at or past P vote false (they load nothing), so the tail word's high bits are zero.  Lane (w mod 64)
// keeps word w and the wave stores up to 64 words at once.
__global__ __launch_bounds__(256) void mask_binarize_kernel(const float* __restrict__ x, int64_t rows, int P, int W, float threshold,
                                                            unsigned long long* __restrict__ bits, int32_t* __restrict__ area) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < rows; r += nwaves) {      // wave-uniform: every lane of a wave reaches every ballot
        const float* row = x + r * P;
        unsigned long long* out = bits + r * W;
        unsigned long long mine = 0ull;
        int a = 0;
        for (int w = 0; w < W; ++w) {
            const int64_t p = (int64_t)64 * w + lane;
            const bool on = p < P && row[p] > threshold;      // NaN > threshold is false
            const unsigned long long word = __ballot(on);
            a += __popcll(word);
            if ((w & 63) == lane) mine = word;
            if ((w & 63) == 63 || w == W - 1) {
                const int first = w & ~63;
                if (first + lane <= w) out[first + lane] = mine;
            }
        }
        if (lane == 0) area[r] = a;
    }
}

// One workgroup per image, one wave per threshold: det_match_kernel (detmetric.hip) with the boxes replaced by packed masks.
// LDS (dynamic; N and M rounded up to 4, so every 4-byte carve is a multiple of 16 bytes): scores, labels, order, tp words, det
// areas, gt labels (-1 = not a ground truth), gt areas, keep bytes (rounded up to 8), then the 8-byte carves: det words, gt words.
__global__ __launch_bounds__(1024) void mask_match_kernel(const float* __restrict__ score, const int32_t* __restrict__ label,
                                                          const unsigned long long* __restrict__ det_bits, const int32_t* __restrict__ det_area,
                                                          const int32_t* __restrict__ gt_label, const unsigned long long* __restrict__ gt_bits,
                                                          const int32_t* __restrict__ gt_area, const int32_t* __restrict__ num_objects,
                                                          mask_thresholds thr, int N, int M, int W, int C, int T, int max_dets,
                                                          int32_t* __restrict__ order, uint16_t* __restrict__ tp_bits,
                                                          int32_t* __restrict__ matched_gt, int32_t* __restrict__ gt_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Np = (N + 3) & ~3, Mp = (M + 3) & ~3;
    float* s_score = reinterpret_cast<float*>(smem);
    int* s_label = reinterpret_cast<int*>(s_score + Np);
    int* s_order = s_label + Np;
    unsigned* s_tp = reinterpret_cast<unsigned*>(s_order + Np);
    int* s_area = reinterpret_cast<int*>(s_tp + Np);
    int* g_label = s_area + Np;
    int* g_area = g_label + Mp;
    unsigned char* s_keep = reinterpret_cast<unsigned char*>(g_area + Mp);
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_keep + ((Np + 7) & ~7));
    unsigned long long* g_bits = s_bits + (size_t)Np * W;

    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;

    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_area[n] = det_area[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        s_keep[n] = 0;
    }
    for (int k = tid; k < N * W; k += nthr) s_bits[k] = det_bits[dbase * W + k];
    for (int k = tid; k < M * W; k += nthr) g_bits[k] = gt_bits[gbase * W + k];
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        g_label[m] = real ? gl : -1;
        g_area[m] = gt_area[gbase + m];
        if (real) atomicAdd(&gt_count[gl], 1);
    }
    for (int64_t k = tid; k < (int64_t)T * N; k += nthr) matched_gt[(int64_t)b * T * N + k] = -1;
    __syncthreads();

    // rank by counting: descending score, equal scores in ascending query order (a stable sort, exactly); the same pass
    // counts the detections of the query's own class that come before it
    for (int n = tid; n < N; n += nthr) {
        const float s = s_score[n];
        const int l = s_label[n];
        int rank = 0, crank = 0;
        for (int j = 0; j < N; ++j) {
            const float sj = s_score[j];
            const bool before = sj > s || (sj == s && j < n);
            rank += before ? 1 : 0;
            crank += (before && s_label[j] == l) ? 1 : 0;
        }
        s_order[rank] = n;                       // rank < N.  (NaN scores would collide here: such slots stay -1 and are skipped)
        s_keep[n] = crank < max_dets ? 1 : 0;
    }
    __syncthreads();
    for (int n = tid; n < N; n += nthr) order[dbase + n] = s_order[n];

    const int wave = tid >> 6, lane = tid & 63;
    if (wave < T) {
        const double th = fmin(thr.v[wave], 1.0 - 1e-10);
        int32_t* mrow = matched_gt + ((int64_t)b * T + wave) * N;
        unsigned taken = 0u;                     // bit k: ground truth lane + 64 k is consumed at this threshold (a lane owns its own)
        for (int r = 0; r < N; ++r) {
            const int d = s_order[r];
            if (d < 0 || !s_keep[d]) continue;   // wave-uniform
            const int dl = s_label[d];
            const unsigned long long* dw = s_bits + (size_t)d * W;
            const long long a_det = s_area[d];
            double best = -1.0;
            int bestm = -1;
            for (int k = 0, m = lane; m < M; m += 64, ++k) {
                if (g_label[m] != dl || ((taken >> k) & 1u)) continue;
                const unsigned long long* gw = g_bits + (size_t)m * W;
                long long inter = 0;
                for (int w = 0; w < W; ++w) inter += __popcll(dw[w] & gw[w]);
                const long long uni = a_det + (long long)g_area[m] - inter;
                const double iou = uni > 0 ? (double)inter / (double)uni : 0.0;
                if (iou >= th && iou >= best) { best = iou; bestm = m; }      // ascending m: on equal IoU the larger index stays
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ob = __shfl_xor(best, o, 64);
                const int om = __shfl_xor(bestm, o, 64);
                if (ob > best || (ob == best && om > bestm)) { best = ob; bestm = om; }
            }
            if (bestm >= 0) {
                if ((bestm & 63) == lane) taken |= 1u << (bestm >> 6);
                if (lane == 0) {
                    mrow[d] = bestm;
                    atomicOr(&s_tp[d], 1u << wave);
                }
            }
        }
    }
    __syncthreads();
    for (int n = tid; n < N; n += nthr) tp_bits[dbase + n] = (uint16_t)(s_tp[n] | (s_keep[n] ? MSK_KEEP_BIT : 0u));
}

// ---------------------------------------------------------------------------------------------------------------------
// The full COCO protocol (K17): mask_match_kernel with crowd regions, area ranges and class ranks, as det_match_coco_kernel
// (detmetric.hip) is to det_match_kernel.  mask_match_kernel above is left as it is.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MSK_MAX_A = 4;         // area ranges
constexpr unsigned char MSK_F_KEEP = 1, MSK_F_OUT = 2;       // detection flags: kept; own area outside the range
constexpr unsigned char MSK_G_IGNORE = 1, MSK_G_CROWD = 2;   // ground-truth flags: ignored in the range; crowd (reusable)

// Grid (B, A): one workgroup per image and area range, one wave per threshold.
// LDS (dynamic; N and M rounded up to 4): scores, labels, order, tp words, ig words, det pixel counts, gt labels, gt pixel counts,
// det flag bytes and gt flag bytes (together rounded up to 8), then the 8-byte carves: det words, gt words.
__global__ __launch_bounds__(1024) void mask_match_coco_kernel(const float* __restrict__ score, const int32_t* __restrict__ label,
                                                               const unsigned long long* __restrict__ det_bits, const int32_t* __restrict__ det_pop,
                                                               const int32_t* __restrict__ gt_label, const unsigned long long* __restrict__ gt_bits,
                                                               const int32_t* __restrict__ gt_pop, const uint8_t* __restrict__ gt_crowd,
                                                               const float* __restrict__ gt_area, const int32_t* __restrict__ num_objects,
                                                               const int32_t* __restrict__ image_hw, const double* __restrict__ area_ranges,
                                                               mask_thresholds thr, int B, int N, int M, int P, int W, int C, int T, int max_dets,
                                                               int32_t* __restrict__ order, int32_t* __restrict__ class_rank,
                                                               uint16_t* __restrict__ tp_bits, uint16_t* __restrict__ ig_bits,
                                                               int32_t* __restrict__ matched_gt, int32_t* __restrict__ gt_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Np = (N + 3) & ~3, Mp = (M + 3) & ~3;
    float* s_score = reinterpret_cast<float*>(smem);
    int* s_label = reinterpret_cast<int*>(s_score + Np);
    int* s_order = s_label + Np;
    unsigned* s_tp = reinterpret_cast<unsigned*>(s_order + Np);
    unsigned* s_ig = s_tp + Np;
    int* s_area = reinterpret_cast<int*>(s_ig + Np);
    int* g_label = s_area + Np;
    int* g_area = g_label + Mp;
    unsigned char* s_flag = reinterpret_cast<unsigned char*>(g_area + Mp);
    unsigned char* g_flag = s_flag + Np;
    unsigned long long* s_bits = reinterpret_cast<unsigned long long*>(s_flag + ((Np + Mp + 7) & ~7));
    unsigned long long* g_bits = s_bits + (size_t)Np * W;

    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;
    const int64_t abase = ((int64_t)a * B + b) * N;            // into tp_bits / ig_bits [A,B,N]
    const double scale = (double)image_hw[2 * b] * (double)image_hw[2 * b + 1];
    const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];

    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_area[n] = det_pop[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        s_ig[n] = 0u;
        s_flag[n] = 0;
    }
    for (int k = tid; k < N * W; k += nthr) s_bits[k] = det_bits[dbase * W + k];
    for (int k = tid; k < M * W; k += nthr) g_bits[k] = gt_bits[gbase * W + k];
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        const int pop = gt_pop[gbase + m];
        unsigned char f = 0;
        if (real) {
            const bool crowd = gt_crowd[gbase + m] != 0;
            const double ar = gt_area ? (double)gt_area[gbase + m] : (double)pop * scale / (double)P;
            const bool ignore = crowd || ar < lo || ar > hi;   // both bounds inclusive
            f = (unsigned char)((ignore ? MSK_G_IGNORE : 0) | (crowd ? MSK_G_CROWD : 0));
            if (!ignore) atomicAdd(&gt_count[(int64_t)a * C + gl], 1);
        }
        g_label[m] = real ? gl : -1;
        g_area[m] = pop;
        g_flag[m] = f;
    }
    for (int64_t k = tid; k < (int64_t)T * N; k += nthr) matched_gt[abase * T + k] = -1;
    __syncthreads();

    // rank by counting, as mask_match_kernel does; the detection's rank within its class is an output here
    for (int n = tid; n < N; n += nthr) {
        const float s = s_score[n];
        const int l = s_label[n];
        int rank = 0, crank = 0;
        for (int j = 0; j < N; ++j) {
            const float sj = s_score[j];
            const bool before = sj > s || (sj == s && j < n);
            rank += before ? 1 : 0;
            crank += (before && s_label[j] == l) ? 1 : 0;
        }
        s_order[rank] = n;                       // rank < N.  (NaN scores would collide here: such slots stay -1 and are skipped)
        const double ar = (double)s_area[n] * scale / (double)P;
        s_flag[n] = (unsigned char)((crank < max_dets ? MSK_F_KEEP : 0) | ((ar < lo || ar > hi) ? MSK_F_OUT : 0));
        if (a == 0) class_rank[dbase + n] = crank;
    }
    __syncthreads();
    if (a == 0)
        for (int n = tid; n < N; n += nthr) order[dbase + n] = s_order[n];

    const int wave = tid >> 6, lane = tid & 63;
    if (wave < T) {
        const double th = fmin(thr.v[wave], 1.0 - 1e-10);
        int32_t* mrow = matched_gt + (abase * T + (int64_t)wave * N);
        unsigned taken = 0u;                     // bit k: ground truth lane + 64 k is consumed at this threshold (a lane owns its own)
        for (int r = 0; r < N; ++r) {
            const int d = s_order[r];
            if (d < 0 || !(s_flag[d] & MSK_F_KEEP)) continue;   // wave-uniform
            const int dl = s_label[d];
            const unsigned long long* dw = s_bits + (size_t)d * W;
            const long long a_det = s_area[d];
            // phase 0: the non-ignored ground truths; phase 1, only when phase 0 found none: the ignored ones.  `phase` and `bestm`
            // after the butterfly are the same in every lane, so the whole wave takes the same path into each reduction.
            double best = -1.0;
            int bestm = -1;
            for (int phase = 0; phase < 2 && bestm < 0; ++phase) {
                best = -1.0;
                for (int k = 0, m = lane; m < M; m += 64, ++k) {
                    if (g_label[m] != dl) continue;
                    const unsigned f = g_flag[m];
                    if ((int)(f & MSK_G_IGNORE) != phase) continue;
                    const bool crowd = (f & MSK_G_CROWD) != 0;
                    if (((taken >> k) & 1u) && !crowd) continue;
                    const unsigned long long* gw = g_bits + (size_t)m * W;
                    long long inter = 0;
                    for (int w = 0; w < W; ++w) inter += __popcll(dw[w] & gw[w]);
                    const long long uni = crowd ? a_det : a_det + (long long)g_area[m] - inter;
                    const double iou = uni > 0 ? (double)inter / (double)uni : 0.0;
                    if (iou >= th && iou >= best) { best = iou; bestm = m; }      // ascending m: on equal IoU the larger index stays
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const double ob = __shfl_xor(best, o, 64);
                    const int om = __shfl_xor(bestm, o, 64);
                    if (ob > best || (ob == best && om > bestm)) { best = ob; bestm = om; }
                }
            }
            if (bestm >= 0) {
                if ((bestm & 63) == lane) taken |= 1u << (bestm >> 6);
                if (lane == 0) {
                    mrow[d] = bestm;
                    if (g_flag[bestm] & MSK_G_IGNORE) atomicOr(&s_ig[d], 1u << wave);
                    else atomicOr(&s_tp[d], 1u << wave);
                }
            } else if (lane == 0 && (s_flag[d] & MSK_F_OUT)) {
                atomicOr(&s_ig[d], 1u << wave);
            }
        }
    }
    __syncthreads();
    for (int n = tid; n < N; n += nthr) {
        tp_bits[abase + n] = (uint16_t)(s_tp[n] | ((s_flag[n] & MSK_F_KEEP) ? MSK_KEEP_BIT : 0u));
        ig_bits[abase + n] = (uint16_t)s_ig[n];
    }
}

}  // namespace

extern "C" int bdetr_mask_binarize(const float* x, int64_t rows, int P, float threshold, uint64_t* bits, int32_t* area, void* stream) {
    BDETR_CHECK_ARG(x && bits && area, "bdetr_mask_binarize: null pointer");
    BDETR_CHECK_ARG(rows > 0 && P > 0, "bdetr_mask_binarize: bad sizes rows=%lld P=%d", (long long)rows, P);
    const int W = (int)(((int64_t)P + 63) / 64);
    int64_t grid = cdiv64(rows, 4);              // four waves (rows) per workgroup
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(mask_binarize_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, rows, P, W, threshold,
                       reinterpret_cast<unsigned long long*>(bits), area);
    return bdetr_launch_status("mask_binarize");
}

extern "C" int bdetr_mask_match(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_area,
                                const int32_t* gt_label, const uint64_t* gt_bits, const int32_t* gt_area, const int32_t* num_objects,
                                const double* thresholds, int B, int N, int M, int W, int C, int T, int max_dets,
                                int32_t* order, uint16_t* tp_bits, int32_t* matched_gt, int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && det_bits && det_area && gt_label && gt_bits && gt_area && num_objects && thresholds && order && tp_bits &&
                    matched_gt && gt_count, "bdetr_mask_match: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && N <= MSK_MAX_N && M > 0 && M <= MSK_MAX_M && W > 0 && C >= 3 && C <= MSK_MAX_C && T > 0 && T <= MSK_MAX_T && max_dets > 0,
                    "bdetr_mask_match: bad sizes B=%d N=%d M=%d W=%d C=%d T=%d max_dets=%d (limits: N <= %d, M <= %d, W >= 1, C in [3, %d], T in [1, %d], max_dets >= 1)",
                    B, N, M, W, C, T, max_dets, MSK_MAX_N, MSK_MAX_M, MSK_MAX_C, MSK_MAX_T);
    const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
    const size_t lds = Np * 20 + Mp * 8 + ((Np + 7) & ~(size_t)7) + 8 * (size_t)W * (Np + Mp);
    BDETR_CHECK_ARG(lds <= MSK_LDS_LIMIT,
                    "bdetr_mask_match: N=%d M=%d W=%d need %zu bytes of LDS per image (%zu of them the packed masks, 8 W (N + M)); the limit is %zu",
                    N, M, W, lds, 8 * (size_t)W * (Np + Mp), MSK_LDS_LIMIT);
    mask_thresholds thr;
    for (int t = 0; t <= MSK_MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : 2.0;
    hipLaunchKernelGGL(mask_match_kernel, dim3(B), dim3(64 * T), lds, (hipStream_t)stream, score, label,
                       reinterpret_cast<const unsigned long long*>(det_bits), det_area, gt_label,
                       reinterpret_cast<const unsigned long long*>(gt_bits), gt_area, num_objects, thr,
                       N, M, W, C, T, max_dets, order, tp_bits, matched_gt, gt_count);
    return bdetr_launch_status("mask_match");
}

extern "C" int bdetr_mask_match_coco(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_pop,
                                     const int32_t* gt_label, const uint64_t* gt_bits, const int32_t* gt_pop, const uint8_t* gt_crowd,
                                     const float* gt_area, const int32_t* num_objects, const int32_t* image_hw, const double* area_ranges,
                                     const double* thresholds, int B, int N, int M, int P, int C, int T, int A, int max_dets,
                                     int32_t* order, int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt,
                                     int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && det_bits && det_pop && gt_label && gt_bits && gt_pop && gt_crowd && num_objects && image_hw && area_ranges &&
                    thresholds && order && class_rank && tp_bits && ig_bits && matched_gt && gt_count,
                    "bdetr_mask_match_coco: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MSK_MAX_N && M > 0 && M <= MSK_MAX_M && P > 0 && C >= 3 && C <= MSK_MAX_C && T > 0 &&
                    T <= MSK_MAX_T && A > 0 && A <= MSK_MAX_A && max_dets > 0,
                    "bdetr_mask_match_coco: bad sizes B=%d N=%d M=%d P=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, P >= 1, "
                    "C in [3, %d], T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, P, C, T, A, max_dets, MSK_MAX_N, MSK_MAX_M, MSK_MAX_C,
                    MSK_MAX_T, MSK_MAX_A);
    const size_t W = ((size_t)P + 63) / 64;
    const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
    const size_t lds = Np * 24 + Mp * 8 + ((Np + Mp + 7) & ~(size_t)7) + 8 * W * (Np + Mp);
    BDETR_CHECK_ARG(lds <= MSK_LDS_LIMIT,
                    "bdetr_mask_match_coco: N=%d M=%d P=%d (W=%zu) need %zu bytes of LDS per image (%zu of them the packed masks, 8 W (N + M)); the limit is %zu",
                    N, M, P, W, lds, 8 * W * (Np + Mp), MSK_LDS_LIMIT);
    mask_thresholds thr;
    for (int t = 0; t <= MSK_MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : 2.0;
    hipLaunchKernelGGL(mask_match_coco_kernel, dim3(B, A), dim3(64 * T), lds, (hipStream_t)stream, score, label,
                       reinterpret_cast<const unsigned long long*>(det_bits), det_pop, gt_label,
                       reinterpret_cast<const unsigned long long*>(gt_bits), gt_pop, gt_crowd, gt_area, num_objects, image_hw, area_ranges, thr,
                       B, N, M, P, (int)W, C, T, max_dets, order, class_rank, tp_bits, ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("mask_match_coco");
}
