// detmetric.hip - on-GPU detection matching for COCO-style box AP on gfx950: every query becomes a detection
// (score, label), and per image the detections are ranked, truncated per class and matched to the ground truths
// at every IoU threshold with COCOeval's greedy rule (no crowd, all areas).  What is left for the host is the
// accumulate over a few bytes per detection (evaluation.py).
//
// Compiled with -ffp-contract=off, as matcher.hip is: the fp64 IoU must be the one an unfused NumPy fp64
// evaluation gives, bit for bit - a match decided at `iou >= threshold` flips on the last bit.
#include "common.h"

namespace {

constexpr int DET_MAX_N = 1024;      // queries per image (LDS: 29 bytes each)
constexpr int DET_MAX_M = 1024;      // ground-truth rows per image (LDS: 20 bytes each; 16 matched bits per lane)
constexpr int DET_MAX_C = 65536;     // classes
constexpr int DET_MAX_T = 15;        // thresholds: bits 0..14 of tp_bits, bit 15 = keep
constexpr unsigned DET_KEEP_BIT = 0x8000u;

struct det_thresholds { double v[DET_MAX_T + 1]; };

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

// One workgroup per image, one wave per threshold.
// LDS (dynamic, every carve a multiple of 16 bytes when N and M are rounded up to 4): det boxes, gt boxes, scores, labels,
// order, tp words, gt labels (-1 = not a ground truth), keep bytes.
__global__ __launch_bounds__(1024) void det_match_kernel(const float* __restrict__ score, const int32_t* __restrict__ label, const float* __restrict__ box_pred,
                                                         const int32_t* __restrict__ gt_label, const float* __restrict__ gt_box,
                                                         const int32_t* __restrict__ num_objects, det_thresholds thr, int N, int M, int C, int T,
                                                         int max_dets, int32_t* __restrict__ order, uint16_t* __restrict__ tp_bits,
                                                         int32_t* __restrict__ matched_gt, int32_t* __restrict__ gt_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Np = (N + 3) & ~3, Mp = (M + 3) & ~3;
    float* s_box = reinterpret_cast<float*>(smem);
    float* g_box = s_box + 4 * Np;
    float* s_score = g_box + 4 * Mp;
    int* s_label = reinterpret_cast<int*>(s_score + Np);
    int* s_order = s_label + Np;
    unsigned* s_tp = reinterpret_cast<unsigned*>(s_order + Np);
    int* g_label = reinterpret_cast<int*>(s_tp + Np);
    unsigned char* s_keep = reinterpret_cast<unsigned char*>(g_label + Mp);

    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;

    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        s_keep[n] = 0;
    }
    for (int k = tid; k < 4 * N; k += nthr) s_box[k] = box_pred[dbase * 4 + k];
    for (int k = tid; k < 4 * M; k += nthr) g_box[k] = gt_box[gbase * 4 + k];
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        g_label[m] = real ? gl : -1;
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
            const double dx0 = (double)s_box[4 * d + 0], dy0 = (double)s_box[4 * d + 1];
            const double dw = fmax((double)s_box[4 * d + 2], 0.0), dh = fmax((double)s_box[4 * d + 3], 0.0);
            const double dx1 = dx0 + dw, dy1 = dy0 + dh;
            const double a_det = dw * dh;
            double best = -1.0;
            int bestm = -1;
            for (int k = 0, m = lane; m < M; m += 64, ++k) {
                if (g_label[m] != dl || ((taken >> k) & 1u)) continue;
                const double gx0 = (double)g_box[4 * m + 0], gy0 = (double)g_box[4 * m + 1];
                const double gw = fmax((double)g_box[4 * m + 2], 0.0), gh = fmax((double)g_box[4 * m + 3], 0.0);
                const double gx1 = gx0 + gw, gy1 = gy0 + gh;
                const double a_gt = gw * gh;
                const double iw = fmax(fmin(dx1, gx1) - fmax(dx0, gx0), 0.0);
                const double ih = fmax(fmin(dy1, gy1) - fmax(dy0, gy0), 0.0);
                const double inter = iw * ih;
                const double uni = (a_det + a_gt) - inter;
                const double iou = uni > 0.0 ? inter / uni : 0.0;
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
    for (int n = tid; n < N; n += nthr) tp_bits[dbase + n] = (uint16_t)(s_tp[n] | (s_keep[n] ? DET_KEEP_BIT : 0u));
}

// ---------------------------------------------------------------------------------------------------------------------
// The full COCO protocol (K16): crowd regions, area ranges, class ranks for several max_dets.  det_match_kernel above is left as
// it is; what follows repeats its staging, ranking and IoU arithmetic line for line and adds the ignore class.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DET_MAX_A = 4;         // area ranges
constexpr unsigned char DET_F_KEEP = 1, DET_F_OUT = 2;       // detection flags: kept; own area outside the range
constexpr unsigned char DET_G_IGNORE = 1, DET_G_CROWD = 2;   // ground-truth flags: ignored in the range; crowd (reusable)

// Grid (B, A): one workgroup per image and area range, one wave per threshold; every workgroup ranks its image again (N^2
// compares out of LDS, cheaper than a second launch and a round trip through HBM).
// LDS (dynamic; N and M rounded up to 4): det boxes, gt boxes, scores, labels, order, tp words, ig words, gt labels, det flag
// bytes, gt flag bytes.
__global__ __launch_bounds__(1024) void det_match_coco_kernel(const float* __restrict__ score, const int32_t* __restrict__ label, const float* __restrict__ box_pred,
                                                              const int32_t* __restrict__ gt_label, const float* __restrict__ gt_box,
                                                              const uint8_t* __restrict__ gt_crowd, const float* __restrict__ gt_area,
                                                              const int32_t* __restrict__ num_objects, const int32_t* __restrict__ image_hw,
                                                              const double* __restrict__ area_ranges, det_thresholds thr, int B, int N, int M, int C, int T,
                                                              int max_dets, int32_t* __restrict__ order, int32_t* __restrict__ class_rank,
                                                              uint16_t* __restrict__ tp_bits, uint16_t* __restrict__ ig_bits,
                                                              int32_t* __restrict__ matched_gt, int32_t* __restrict__ gt_count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int Np = (N + 3) & ~3, Mp = (M + 3) & ~3;
    float* s_box = reinterpret_cast<float*>(smem);
    float* g_box = s_box + 4 * Np;
    float* s_score = g_box + 4 * Mp;
    int* s_label = reinterpret_cast<int*>(s_score + Np);
    int* s_order = s_label + Np;
    unsigned* s_tp = reinterpret_cast<unsigned*>(s_order + Np);
    unsigned* s_ig = s_tp + Np;
    int* g_label = reinterpret_cast<int*>(s_ig + Np);
    unsigned char* s_flag = reinterpret_cast<unsigned char*>(g_label + Mp);
    unsigned char* g_flag = s_flag + Np;

    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;
    const int64_t abase = ((int64_t)a * B + b) * N;            // into tp_bits / ig_bits [A,B,N]
    const double scale = (double)image_hw[2 * b] * (double)image_hw[2 * b + 1];
    const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];

    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        s_ig[n] = 0u;
        s_flag[n] = 0;
    }
    for (int k = tid; k < 4 * N; k += nthr) s_box[k] = box_pred[dbase * 4 + k];
    for (int k = tid; k < 4 * M; k += nthr) g_box[k] = gt_box[gbase * 4 + k];
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        unsigned char f = 0;
        if (real) {
            const bool crowd = gt_crowd[gbase + m] != 0;
            double ar;
            if (gt_area) {
                ar = (double)gt_area[gbase + m];
            } else {
                const double gw = fmax((double)gt_box[(gbase + m) * 4 + 2], 0.0), gh = fmax((double)gt_box[(gbase + m) * 4 + 3], 0.0);
                ar = (gw * gh) * scale;
            }
            const bool ignore = crowd || ar < lo || ar > hi;   // both bounds inclusive
            f = (unsigned char)((ignore ? DET_G_IGNORE : 0) | (crowd ? DET_G_CROWD : 0));
            if (!ignore) atomicAdd(&gt_count[(int64_t)a * C + gl], 1);
        }
        g_label[m] = real ? gl : -1;
        g_flag[m] = f;
    }
    for (int64_t k = tid; k < (int64_t)T * N; k += nthr) matched_gt[abase * T + k] = -1;
    __syncthreads();

    // rank by counting, as det_match_kernel does; the detection's rank within its class is an output here
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
        const double dw = fmax((double)s_box[4 * n + 2], 0.0), dh = fmax((double)s_box[4 * n + 3], 0.0);
        const double ar = (dw * dh) * scale;
        s_flag[n] = (unsigned char)((crank < max_dets ? DET_F_KEEP : 0) | ((ar < lo || ar > hi) ? DET_F_OUT : 0));
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
            if (d < 0 || !(s_flag[d] & DET_F_KEEP)) continue;   // wave-uniform
            const int dl = s_label[d];
            const double dx0 = (double)s_box[4 * d + 0], dy0 = (double)s_box[4 * d + 1];
            const double dw = fmax((double)s_box[4 * d + 2], 0.0), dh = fmax((double)s_box[4 * d + 3], 0.0);
            const double dx1 = dx0 + dw, dy1 = dy0 + dh;
            const double a_det = dw * dh;
            // phase 0: the non-ignored ground truths; phase 1, only when phase 0 found none: the ignored ones (COCOeval sorts the
            // ignored ground truths last and breaks out of its scan on reaching them with a match in hand).  `phase` and `bestm`
            // after the butterfly are the same in every lane, so the whole wave takes the same path into each reduction.
            double best = -1.0;
            int bestm = -1;
            for (int phase = 0; phase < 2 && bestm < 0; ++phase) {
                best = -1.0;
                for (int k = 0, m = lane; m < M; m += 64, ++k) {
                    if (g_label[m] != dl) continue;
                    const unsigned f = g_flag[m];
                    if ((int)(f & DET_G_IGNORE) != phase) continue;
                    const bool crowd = (f & DET_G_CROWD) != 0;
                    if (((taken >> k) & 1u) && !crowd) continue;
                    const double gx0 = (double)g_box[4 * m + 0], gy0 = (double)g_box[4 * m + 1];
                    const double gw = fmax((double)g_box[4 * m + 2], 0.0), gh = fmax((double)g_box[4 * m + 3], 0.0);
                    const double gx1 = gx0 + gw, gy1 = gy0 + gh;
                    const double a_gt = gw * gh;
                    const double iw = fmax(fmin(dx1, gx1) - fmax(dx0, gx0), 0.0);
                    const double ih = fmax(fmin(dy1, gy1) - fmax(dy0, gy0), 0.0);
                    const double inter = iw * ih;
                    const double uni = crowd ? a_det : (a_det + a_gt) - inter;
                    const double iou = uni > 0.0 ? inter / uni : 0.0;
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
                    if (g_flag[bestm] & DET_G_IGNORE) atomicOr(&s_ig[d], 1u << wave);
                    else atomicOr(&s_tp[d], 1u << wave);
                }
            } else if (lane == 0 && (s_flag[d] & DET_F_OUT)) {
                atomicOr(&s_ig[d], 1u << wave);
            }
        }
    }
    __syncthreads();
    for (int n = tid; n < N; n += nthr) {
        tp_bits[abase + n] = (uint16_t)(s_tp[n] | ((s_flag[n] & DET_F_KEEP) ? DET_KEEP_BIT : 0u));
        ig_bits[abase + n] = (uint16_t)s_ig[n];
    }
}

}  // namespace

extern "C" int bdetr_det_postprocess(const float* cat_pred, int B, int N, int C, float* score, int32_t* label, void* stream) {
    BDETR_CHECK_ARG(cat_pred && score && label, "bdetr_det_postprocess: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && C >= 3 && C <= DET_MAX_C, "bdetr_det_postprocess: bad sizes B=%d N=%d C=%d (C in [3, %d])", B, N, C, DET_MAX_C);
    const int64_t rows = (int64_t)B * N;
    hipLaunchKernelGGL(det_postprocess_kernel, dim3(ew_grid(rows, 256, 1)), dim3(256), 0, (hipStream_t)stream, cat_pred, rows, C, score, label);
    return bdetr_launch_status("det_postprocess");
}

extern "C" int bdetr_det_match(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                               const int32_t* num_objects, const double* thresholds, int B, int N, int M, int C, int T, int max_dets,
                               int32_t* order, uint16_t* tp_bits, int32_t* matched_gt, int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && box_pred && gt_label && gt_box && num_objects && thresholds && order && tp_bits && matched_gt && gt_count,
                    "bdetr_det_match: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && N <= DET_MAX_N && M > 0 && M <= DET_MAX_M && C >= 3 && C <= DET_MAX_C && T > 0 && T <= DET_MAX_T && max_dets > 0,
                    "bdetr_det_match: bad sizes B=%d N=%d M=%d C=%d T=%d max_dets=%d (limits: N <= %d, M <= %d, C in [3, %d], T in [1, %d], max_dets >= 1)",
                    B, N, M, C, T, max_dets, DET_MAX_N, DET_MAX_M, DET_MAX_C, DET_MAX_T);
    det_thresholds thr;
    for (int t = 0; t <= DET_MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : 2.0;
    const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
    const size_t lds = Np * (16 + 4 * 4) + Mp * (16 + 4) + Np;      // <= 53 KiB at the limits: inside the default 64 KiB
    hipLaunchKernelGGL(det_match_kernel, dim3(B), dim3(64 * T), lds, (hipStream_t)stream, score, label, box_pred, gt_label, gt_box, num_objects, thr,
                       N, M, C, T, max_dets, order, tp_bits, matched_gt, gt_count);
    return bdetr_launch_status("det_match");
}

extern "C" int bdetr_det_match_coco(const float* score, const int32_t* label, const float* box_pred, const int32_t* gt_label, const float* gt_box,
                                    const uint8_t* gt_crowd, const float* gt_area, const int32_t* num_objects, const int32_t* image_hw,
                                    const double* area_ranges, const double* thresholds, int B, int N, int M, int C, int T, int A, int max_dets,
                                    int32_t* order, int32_t* class_rank, uint16_t* tp_bits, uint16_t* ig_bits, int32_t* matched_gt,
                                    int32_t* gt_count, void* stream) {
    BDETR_CHECK_ARG(score && label && box_pred && gt_label && gt_box && gt_crowd && num_objects && image_hw && area_ranges && thresholds && order &&
                    class_rank && tp_bits && ig_bits && matched_gt && gt_count, "bdetr_det_match_coco: null pointer (only gt_area may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= DET_MAX_N && M > 0 && M <= DET_MAX_M && C >= 3 && C <= DET_MAX_C && T > 0 && T <= DET_MAX_T &&
                    A > 0 && A <= DET_MAX_A && max_dets > 0,
                    "bdetr_det_match_coco: bad sizes B=%d N=%d M=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, C in [3, %d], "
                    "T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, C, T, A, max_dets, DET_MAX_N, DET_MAX_M, DET_MAX_C, DET_MAX_T, DET_MAX_A);
    det_thresholds thr;
    for (int t = 0; t <= DET_MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : 2.0;
    const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
    const size_t lds = Np * (16 + 5 * 4) + Mp * (16 + 4) + Np + Mp;      // 59 KiB at the limits: inside the default 64 KiB
    hipLaunchKernelGGL(det_match_coco_kernel, dim3(B, A), dim3(64 * T), lds, (hipStream_t)stream, score, label, box_pred, gt_label, gt_box, gt_crowd,
                       gt_area, num_objects, image_hw, area_ranges, thr, B, N, M, C, T, max_dets, order, class_rank, tp_bits, ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("det_match_coco");
}
