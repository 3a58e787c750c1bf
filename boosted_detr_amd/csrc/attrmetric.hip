// attrmetric.hip - attribute-aware detection AP on gfx950 (Fashionpedia's AP_IoU+F1, in this project's own words): a detection is a
// true positive only when its IoU with a ground truth reaches the IoU threshold AND the F1 of its predicted attribute set against
// that ground truth's reaches an F1 threshold.  K29 packs attribute rows into 64-bit words (one wave ballot per word, as
// mask_binarize does); K30 and K31 launch coco_match.h's one kernel exactly as K16 and K17 do, with the F1 gate (f1_gate) as its
// third template parameter and one workgroup per (image, area range, F1 threshold).  The host accumulates per F1 threshold as for
// boxes (evaluation.py, AttributeEvaluator).
//
// Compiled with -ffp-contract=off, as detmetric.hip is: see coco_match.h.
#include "coco_match.h"

using namespace cocomatch;

namespace {

constexpr int ATTR_MAX = 64 * MAX_WA;      // 4096 attributes

// One wave per row, as mask_binarize_kernel: lane l of step w holds attribute 64 w + l, the wave's ballot of the predicate is the
// word.  The predicate is the reference's decode rule, x >= 0.5 (NaN >= 0.5 is false), on attributes 2 .. A-1: <PAD> and <OOV> are
// never an attribute.  Lanes at or past A vote false (they load nothing), so the tail word's high bits are zero.  Wa <= 64: lane w
// keeps word w and the wave stores its words at once.
__global__ __launch_bounds__(256) void attr_pack_kernel(const float* __restrict__ x, int64_t rows, int A, int Wa,
                                                        unsigned long long* __restrict__ bits, int32_t* __restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r = wave; r < rows; r += nwaves) {      // wave-uniform: every lane of a wave reaches every ballot
        const float* row = x + r * A;
        unsigned long long mine = 0ull;
        int c = 0;
        for (int w = 0; w < Wa; ++w) {
            const int a = 64 * w + lane;
            const bool on = a >= 2 && a < A && row[a] >= 0.5f;
            const unsigned long long word = __ballot(on);
            c += __popcll(word);
            if (w == lane) mine = word;
        }
        if (lane < Wa) bits[r * Wa + lane] = mine;
        if (lane == 0) count[r] = c;
    }
}

// What K30 and K31 check beyond K16 / K17, and the gate's source.
bool gate_source(const char* what, const uint64_t* det_attr, const int32_t* det_count, const uint64_t* gt_attr, const int32_t* gt_attr_count,
                 const double* f1_thresholds, int Wa, int F, double empty_f1, f1_gate::source* out) {
    if (!(det_attr && det_count && gt_attr && gt_attr_count && f1_thresholds)) {
        bdetr_set_error("%s: null pointer (only gt_area may be null)", what);
        return false;
    }
    if (!(F > 0 && F <= MAX_F && Wa > 0 && Wa <= MAX_WA && (empty_f1 == 0.0 || empty_f1 == 1.0))) {
        bdetr_set_error("%s: bad gate F=%d Wa=%d empty_f1=%g (limits: F in [1, %d], Wa in [1, %d], empty_f1 0 or 1)", what, F, Wa, empty_f1, MAX_F,
                        MAX_WA);
        return false;
    }
    out->det_attr = reinterpret_cast<const unsigned long long*>(det_attr);
    out->det_count = det_count;
    out->gt_attr = reinterpret_cast<const unsigned long long*>(gt_attr);
    out->gt_count = gt_attr_count;
    out->Wa = Wa;
    out->empty_f1 = empty_f1;
    for (int f = 0; f < MAX_F; ++f) out->thr[f] = f < F ? f1_thresholds[f] : 2.0;
    return true;
}

}  // namespace

extern "C" int bdetr_attr_pack(const float* x, int64_t rows, int A, uint64_t* bits, int32_t* count, void* stream) {
    BDETR_CHECK_ARG(x && bits && count, "bdetr_attr_pack: null pointer");
    BDETR_CHECK_ARG(rows > 0 && A >= 3 && A <= ATTR_MAX, "bdetr_attr_pack: bad sizes rows=%lld A=%d (A in [3, %d])", (long long)rows, A, ATTR_MAX);
    const int Wa = (A + 63) / 64;
    int64_t grid = cdiv64(rows, 4);              // four waves (rows) per workgroup
    if (grid > 2048) grid = 2048;
    hipLaunchKernelGGL(attr_pack_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, rows, A, Wa,
                       reinterpret_cast<unsigned long long*>(bits), count);
    return bdetr_launch_status("attr_pack");
}

extern "C" int bdetr_det_match_attr(const float* score, const int32_t* label, const float* box_pred, const uint64_t* det_attr,
                                    const int32_t* det_count, const int32_t* gt_label, const float* gt_box, const uint64_t* gt_attr,
                                    const int32_t* gt_attr_count, const uint8_t* gt_crowd, const float* gt_area, const int32_t* num_objects,
                                    const int32_t* image_hw, const double* area_ranges, const double* thresholds, const double* f1_thresholds,
                                    double empty_f1, int B, int N, int M, int C, int Wa, int T, int F, int A, int max_dets, int32_t* order,
                                    int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count,
                                    void* stream) {
    BDETR_CHECK_ARG(score && label && box_pred && gt_label && gt_box && gt_crowd && num_objects && image_hw && area_ranges && thresholds && order &&
                    class_rank && tp_bits && ig_bits && matched_gt && gt_count, "bdetr_det_match_attr: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && C >= 3 && C <= MAX_C && T > 0 && T <= MAX_T &&
                    A > 0 && A <= MAX_A && max_dets > 0,
                    "bdetr_det_match_attr: bad sizes B=%d N=%d M=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, C in [3, %d], "
                    "T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, C, T, A, max_dets, MAX_N, MAX_M, MAX_C, MAX_T, MAX_A);
    f1_gate::source gsrc;
    if (!gate_source("bdetr_det_match_attr", det_attr, det_count, gt_attr, gt_attr_count, f1_thresholds, Wa, F, empty_f1, &gsrc)) return -1;
    const box_iou::source src = {box_pred, gt_box};
    const carve<box_iou, true, f1_gate> at(N, M, src, gsrc);
    BDETR_CHECK_ARG(at.total <= LDS_LIMIT,
                    "bdetr_det_match_attr: N=%d M=%d Wa=%d need %zu bytes of LDS per image (%zu of them the attribute sets, (8 Wa + 4) (N + M)); the "
                    "limit is %zu", N, M, Wa, at.total, at.total - at.gate, LDS_LIMIT);
    hipLaunchKernelGGL((coco_match_kernel<box_iou, true, f1_gate>), dim3(B, A, F), dim3(64 * T), at.total, (hipStream_t)stream, src, score, label,
                       gt_label, gt_crowd, gt_area, num_objects, image_hw, area_ranges, match_thresholds(thresholds, T), B, N, M, C, T, max_dets,
                       order, class_rank, tp_bits, ig_bits, matched_gt, gt_count, gsrc);
    return bdetr_launch_status("det_match_attr");
}

extern "C" int bdetr_mask_match_attr(const float* score, const int32_t* label, const uint64_t* det_bits, const int32_t* det_pop,
                                     const uint64_t* det_attr, const int32_t* det_count, const int32_t* gt_label, const uint64_t* gt_bits,
                                     const int32_t* gt_pop, const uint64_t* gt_attr, const int32_t* gt_attr_count, const uint8_t* gt_crowd,
                                     const float* gt_area, const int32_t* num_objects, const int32_t* image_hw, const double* area_ranges,
                                     const double* thresholds, const double* f1_thresholds, double empty_f1, int B, int N, int M, int P, int C,
                                     int Wa, int T, int F, int A, int max_dets, int32_t* order, int32_t* class_rank, uint16_t* tp_bits,
                                     uint16_t* ig_bits, int32_t* matched_gt, int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && det_bits && det_pop && gt_label && gt_bits && gt_pop && gt_crowd && num_objects && image_hw && area_ranges &&
                    thresholds && order && class_rank && tp_bits && ig_bits && matched_gt && gt_count,
                    "bdetr_mask_match_attr: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N && M > 0 && M <= MAX_M && P > 0 && C >= 3 && C <= MAX_C && T > 0 &&
                    T <= MAX_T && A > 0 && A <= MAX_A && max_dets > 0,
                    "bdetr_mask_match_attr: bad sizes B=%d N=%d M=%d P=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, P >= 1, "
                    "C in [3, %d], T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, P, C, T, A, max_dets, MAX_N, MAX_M, MAX_C,
                    MAX_T, MAX_A);
    f1_gate::source gsrc;
    if (!gate_source("bdetr_mask_match_attr", det_attr, det_count, gt_attr, gt_attr_count, f1_thresholds, Wa, F, empty_f1, &gsrc)) return -1;
    const size_t W = ((size_t)P + 63) / 64;
    const words_iou::source src = {reinterpret_cast<const unsigned long long*>(det_bits), det_pop,
                                   reinterpret_cast<const unsigned long long*>(gt_bits), gt_pop, P, (int)W};
    const carve<words_iou, true, f1_gate> at(N, M, src, gsrc);
    BDETR_CHECK_ARG(at.total <= LDS_LIMIT,
                    "bdetr_mask_match_attr: N=%d M=%d P=%d (W=%zu) Wa=%d need %zu bytes of LDS per image (%zu of them the packed masks, 8 W (N + M), "
                    "%zu the attribute sets, (8 Wa + 4) (N + M)); the limit is %zu", N, M, P, W, Wa, at.total, at.gate - at.tail, at.total - at.gate,
                    LDS_LIMIT);
    hipLaunchKernelGGL((coco_match_kernel<words_iou, true, f1_gate>), dim3(B, A, F), dim3(64 * T), at.total, (hipStream_t)stream, src, score, label,
                       gt_label, gt_crowd, gt_area, num_objects, image_hw, area_ranges, match_thresholds(thresholds, T), B, N, M, C, T, max_dets,
                       order, class_rank, tp_bits, ig_bits, matched_gt, gt_count, gsrc);
    return bdetr_launch_status("mask_match_attr");
}
