// maskmetric.hip - on-GPU mask matching for COCO-style mask AP (pycocotools' iouType="segm") on gfx950: masks are packed into
// 64-bit words (one wave ballot per word, mask_binarize), and the entry points of the mask matchers K15 and K17 launch
// coco_match.h's one kernel exactly as detmetric.hip does for boxes - only the IoU source differs: popcounts of packed words
// (words_iou) instead of box corners.  The host accumulates as for boxes (evaluation.py).
//
// Compiled with -ffp-contract=off, as detmetric.hip is: see coco_match.h.
#include "coco_match.h"

using namespace cocomatch;

namespace {

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
    BDETR_CHECK_ARG(B > 0 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && W > 0 && C >= 3 && C <= MAX_C && T > 0 && T <= MAX_T && max_dets > 0,
                    "bdetr_mask_match: bad sizes B=%d N=%d M=%d W=%d C=%d T=%d max_dets=%d (limits: N <= %d, M <= %d, W >= 1, C in [3, %d], T in [1, %d], max_dets >= 1)",
                    B, N, M, W, C, T, max_dets, MAX_N, MAX_M, MAX_C, MAX_T);
    const words_iou::source src = {reinterpret_cast<const unsigned long long*>(det_bits), det_area,
                                   reinterpret_cast<const unsigned long long*>(gt_bits), gt_area, 0, W};
    const carve<words_iou, false> at(N, M, src);
    BDETR_CHECK_ARG(at.total <= LDS_LIMIT,
                    "bdetr_mask_match: N=%d M=%d W=%d need %zu bytes of LDS per image (%zu of them the packed masks, 8 W (N + M)); the limit is %zu",
                    N, M, W, at.total, at.total - at.tail, LDS_LIMIT);
    hipLaunchKernelGGL((coco_match_kernel<words_iou, false>), dim3(B), dim3(64 * T), at.total, (hipStream_t)stream, src, score, label, gt_label,
                       nullptr, nullptr, num_objects, nullptr, nullptr, match_thresholds(thresholds, T), B, N, M, C, T, max_dets, order, nullptr,
                       tp_bits, nullptr, matched_gt, gt_count);
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
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && P > 0 && C >= 3 && C <= MAX_C && T > 0 &&
                    T <= MAX_T && A > 0 && A <= MAX_A && max_dets > 0,
                    "bdetr_mask_match_coco: bad sizes B=%d N=%d M=%d P=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, P >= 1, "
                    "C in [3, %d], T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, P, C, T, A, max_dets, MAX_N, MAX_M, MAX_C,
                    MAX_T, MAX_A);
    const size_t W = ((size_t)P + 63) / 64;
    const words_iou::source src = {reinterpret_cast<const unsigned long long*>(det_bits), det_pop,
                                   reinterpret_cast<const unsigned long long*>(gt_bits), gt_pop, P, (int)W};
    const carve<words_iou, true> at(N, M, src);
    BDETR_CHECK_ARG(at.total <= LDS_LIMIT,
                    "bdetr_mask_match_coco: N=%d M=%d P=%d (W=%zu) need %zu bytes of LDS per image (%zu of them the packed masks, 8 W (N + M)); the limit is %zu",
                    N, M, P, W, at.total, at.total - at.tail, LDS_LIMIT);
    hipLaunchKernelGGL((coco_match_kernel<words_iou, true>), dim3(B, A), dim3(64 * T), at.total, (hipStream_t)stream, src, score, label, gt_label,
                       gt_crowd, gt_area, num_objects, image_hw, area_ranges, match_thresholds(thresholds, T), B, N, M, C, T, max_dets, order,
                       class_rank, tp_bits, ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("mask_match_coco");
}
