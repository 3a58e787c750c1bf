// detmetric.hip - on-GPU detection matching for COCO-style box AP on gfx950: the post-processing that turns every query into a
// detection (score, label), and the entry points of the box matchers - K14 (no crowd, all areas) and K16 (the full COCO protocol:
// crowd regions, area ranges, class ranks for several max_dets).  The matching itself is coco_match.h's one kernel with the box
// IoU source (box_iou); what is left for the host is the accumulate over a few bytes per detection (evaluation.py).
//
// Compiled with -ffp-contract=off, as matcher.hip is: see coco_match.h.
#include "coco_match.h"

using namespace cocomatch;

namespace {

// label = first-max argmax over classes 2 .. C-1 (<PAD> and <OOV> are never a detection), score = that probability
__global__ void det_postprocess_kernel(const float* __restrict__ cat_pred, int64_t rows, int C, float* __restrict__ score, int32_t* __restrict__ label) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const float* p = cat_pred + r * C;
        float best = p[2];
        int bl = 2;
        for (int c = 3; c < C; ++c) {
            const float v = p[c];
            if (v > best) { best = v; bl = c; }
        }
        score[r] = best;
        label[r] = bl;
    }
}

}  // namespace

extern "C" int bdetr_det_postprocess(const float* cat_pred, int B, int N, int C, float* score, int32_t* label, void* stream) {
    BDETR_CHECK_ARG(cat_pred && score && label, "bdetr_det_postprocess: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && C >= 3 && C <= MAX_C, "bdetr_det_postprocess: bad sizes B=%d N=%d C=%d (C in [3, %d])", B, N, C, MAX_C);
    const int64_t rows = (int64_t)B * N;
    hipLaunchKernelGGL(det_postprocess_kernel, dim3(ew_grid(rows, 256, 1)), dim3(256), 0, (hipStream_t)stream, cat_pred, rows, C, score, label);
    return bdetr_launch_status("det_postprocess");
}

extern "C" int bdetr_det_match(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                               const int32_t* num_objects, const double* thresholds, int B, int N, int M, int C, int T, int max_dets,
                               int32_t* order, uint16_t* tp_bits, int32_t* matched_gt, int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && box_pred && gt_label && gt_box && num_objects && thresholds && order && tp_bits && matched_gt && gt_count,
                    "bdetr_det_match: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && C >= 3 && C <= MAX_C && T > 0 && T <= MAX_T && max_dets > 0,
                    "bdetr_det_match: bad sizes B=%d N=%d M=%d C=%d T=%d max_dets=%d (limits: N <= %d, M <= %d, C in [3, %d], T in [1, %d], max_dets >= 1)",
                    B, N, M, C, T, max_dets, MAX_N, MAX_M, MAX_C, MAX_T);
    const box_iou::source src = {box_pred, gt_box};
    const size_t lds = carve<box_iou, false>(N, M, src).total;      // 29 bytes a query, 20 a ground truth: <= 53 KiB, inside the default 64 KiB
    hipLaunchKernelGGL((coco_match_kernel<box_iou, false>), dim3(B), dim3(64 * T), lds, (hipStream_t)stream, src, score, label, gt_label, nullptr,
                       nullptr, num_objects, nullptr, nullptr, match_thresholds(thresholds, T), B, N, M, C, T, max_dets, order, nullptr, tp_bits,
                       nullptr, matched_gt, gt_count);
    return bdetr_launch_status("det_match");
}

extern "C" int bdetr_det_match_coco(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                                    const uint8_t* gt_crowd, const float* gt_area, const int32_t* num_objects, const int32_t* image_hw,
                                    const double* area_ranges, const double* thresholds, int B, int N, int M, int C, int T, int A, int max_dets,
                                    int32_t* order, int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt,
                                    int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && box_pred && gt_label && gt_box && gt_crowd && num_objects && image_hw && area_ranges && thresholds && order &&
                    class_rank && tp_bits && ig_bits && matched_gt && gt_count, "bdetr_det_match_coco: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && C >= 3 && C <= MAX_C && T > 0 && T <= MAX_T &&
                    A > 0 && A <= MAX_A && max_dets > 0,
                    "bdetr_det_match_coco: bad sizes B=%d N=%d M=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, C in [3, %d], "
                    "T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, C, T, A, max_dets, MAX_N, MAX_M, MAX_C, MAX_T, MAX_A);
    const box_iou::source src = {box_pred, gt_box};
    const size_t lds = carve<box_iou, true>(N, M, src).total;       // 59 KiB at the limits: inside the default 64 KiB
    hipLaunchKernelGGL((coco_match_kernel<box_iou, true>), dim3(B, A), dim3(64 * T), lds, (hipStream_t)stream, src, score, label, gt_label, gt_crowd,
                       gt_area, num_objects, image_hw, area_ranges, match_thresholds(thresholds, T), B, N, M, C, T, max_dets, order, class_rank,
                       tp_bits, ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("det_match_coco");
}
