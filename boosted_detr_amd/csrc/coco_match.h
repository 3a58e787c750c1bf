// coco_match.h - COCOeval's greedy matching on gfx950, written once: every query becomes a detection (score, label), and per
// image the detections are ranked, truncated per class and matched to the ground truths at every IoU threshold.  What is left
// for the host is the accumulate over a few bytes per detection (evaluation.py).  Four translation units launch it:
//   detmetric.hip   K14 / K16  coco_match_kernel<box_iou, false / true>           IoU of box corners in fp64
//   maskmetric.hip  K15 / K17  coco_match_kernel<words_iou, false / true>         popcounts of packed mask words in LDS
//   maskimage.hip   K22        coco_match_kernel<inter_iou<STAGED>, true>         a precomputed inter [N,M] (K21), in LDS or in HBM
//   attrmetric.hip  K30 / K31  coco_match_kernel<box_iou / words_iou, true, f1_gate>   K16 / K17 with the attribute F1 gate
// `COCO` is the full protocol - crowd regions, area ranges, class ranks for several max_dets: the ignore class.  Without it the
// phase loop, the ig words, the ground truths' flag bytes, class_rank, the area flags and the (B, A) grid are compiled out, so
// the plain kernels keep their registers and their LDS.  An IoU source is a struct with only what differs (see box_iou).
// `Gate` is one more test a ground truth has to pass to be a candidate (see no_gate / f1_gate); the default, no_gate, has an empty
// source, no LDS and a pass() that is true, so for the five kernels without one the promise above covers the gate as well.
//
// Exactness does not depend on who includes this: no a*b+c below is contracted into an fma, so the fp64 IoU is the one an unfused
// NumPy fp64 evaluation gives, bit for bit - a match decided at `iou >= threshold` flips on the last bit.  (build.py also passes
// -ffp-contract=off for the three files.)
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace cocomatch {

constexpr int MAX_N = 1024;      // queries per image
constexpr int MAX_M = 1024;      // ground-truth rows per image (16 matched bits per lane)
constexpr int MAX_C = 65536;     // classes
constexpr int MAX_T = 15;        // thresholds: bits 0..14 of tp_bits, bit 15 = keep
constexpr int MAX_A = 4;         // area ranges
constexpr int MAX_F = 16;        // F1 thresholds of the attribute gate: blockIdx.z
constexpr int MAX_WA = 64;       // 64-bit words of an attribute set (4096 attributes)
constexpr unsigned KEEP_BIT = 0x8000u;
constexpr size_t LDS_LIMIT = 64 * 1024;      // the default dynamic LDS of a workgroup (no opt-in to the CU's 160 KiB)
constexpr unsigned char F_KEEP = 1, F_OUT = 2;       // detection flags: kept; own area outside the range
constexpr unsigned char G_IGNORE = 1, G_CROWD = 2;   // ground-truth flags: ignored in the range; crowd (reusable)

struct match_thresholds {
    double v[MAX_T + 1];
    match_thresholds(const double* host, int T) {
        for (int t = 0; t <= MAX_T; ++t) v[t] = t < T ? host[t] : 2.0;
    }
};

// A gate is a struct like an IoU source: `source` (its operands, a kernel argument), ON, its share of the LDS (TAIL_ALIGN, bytes),
// stage(src, f, b, ...) (carve that share and fill it, before the kernel's first synchronise; f = blockIdx.z selects the gate's own
// threshold), begin(d) (the per-detection set-up) and pass(m): whether ground truth m may be matched to detection d at all.
struct no_gate {
    struct source {};
    static constexpr bool ON = false;
    static constexpr unsigned TAIL_ALIGN = 1;
    static __host__ __device__ size_t bytes(size_t, size_t, const source&) { return 0; }
    __device__ __forceinline__ void stage(const source&, int, int, int, int, unsigned char*, int, int) {}
    __device__ __forceinline__ void begin(int) {}
    __device__ __forceinline__ bool pass(int) const { return true; }
};

// The attribute F1 gate (K30 / K31): det_attr [B,N,Wa] / det_count [B,N] and gt_attr [B,M,Wa] / gt_count [B,M] as bdetr_attr_pack
// (K29) leaves them.  F1 = 2 tp / (count_d + count_g) with tp the popcount of the common bits: ONE IEEE fp64 division of exact
// integers, as the mask IoU is, so equal rationals are equal doubles and 2 * 1 / (2 + 2) meets 0.5; two empty sets score empty_f1.
// LDS: det words, gt words, then det counts, gt counts.
struct f1_gate {
    struct source {
        const unsigned long long* det_attr;
        const int32_t* det_count;
        const unsigned long long* gt_attr;
        const int32_t* gt_count;
        int Wa;
        double empty_f1;
        double thr[MAX_F];
    };
    static constexpr bool ON = true;
    static constexpr unsigned TAIL_ALIGN = 8;
    static __host__ __device__ size_t bytes(size_t Np, size_t Mp, const source& src) { return (8 * (size_t)src.Wa + 4) * (Np + Mp); }

    const unsigned long long *s_bits, *g_bits, *dw;
    const int *s_cnt, *g_cnt;
    int Wa, dcount;
    double th, empty;

    __device__ __forceinline__ void stage(const source& src, int f, int b, int N, int M, unsigned char* at, int tid, int nthr) {
        const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
        Wa = src.Wa;
        th = fmin(src.thr[f], 1.0 - 1e-10);
        empty = src.empty_f1;
        unsigned long long* sb = reinterpret_cast<unsigned long long*>(at);
        unsigned long long* gb = sb + Np * Wa;
        int* sc = reinterpret_cast<int*>(gb + Mp * Wa);
        int* gc = sc + Np;
        for (int k = tid; k < N * Wa; k += nthr) sb[k] = src.det_attr[(int64_t)b * N * Wa + k];
        for (int k = tid; k < M * Wa; k += nthr) gb[k] = src.gt_attr[(int64_t)b * M * Wa + k];
        for (int k = tid; k < N; k += nthr) sc[k] = src.det_count[(int64_t)b * N + k];
        for (int k = tid; k < M; k += nthr) gc[k] = src.gt_count[(int64_t)b * M + k];
        s_bits = sb;
        g_bits = gb;
        s_cnt = sc;
        g_cnt = gc;
    }
    __device__ __forceinline__ void begin(int d) {
        dw = s_bits + (size_t)d * Wa;
        dcount = s_cnt[d];
    }
    __device__ __forceinline__ bool pass(int m) const {
        const unsigned long long* gw = g_bits + (size_t)m * Wa;
        int tp = 0;
        for (int w = 0; w < Wa; ++w) tp += __popcll(dw[w] & gw[w]);
        const int both = dcount + g_cnt[m];
        const double f1 = both > 0 ? (double)(2 * tp) / (double)both : empty;
        return f1 >= th;
    }
};

// The dynamic LDS of coco_match_kernel<Iou, COCO, Gate>, as byte offsets; the entry points size the launch with the same object the
// kernel carves with.  N and M are rounded up to 4, so every 4-byte carve is a multiple of 16 bytes:
//   [0, words)       scores, labels, order, tp words (COCO: ig words) [N]; gt labels [M] (-1 = not a ground truth)
//   [words, flags)   the source's 4- and 16-byte carves
//   [flags, tail)    det flag bytes [N] (COCO: gt flag bytes [M]), rounded up to the source's (and the gate's) TAIL_ALIGN
//   [tail, gate)     the source's 8-byte carves (with a gate rounded up to 8 bytes)
//   [gate, total)    the gate's carves; nothing without one
// The offsets are 32-bit on purpose (at most 61 KiB before the tail): from 64-bit arithmetic the compiler no longer sees the carves'
// 16- and 8-byte alignment and splits a box's one 16-byte LDS read in the matching loop.  Only the tail's size can be large.
template <class Iou, bool COCO, class Gate = no_gate>
struct carve {
    unsigned words, flags, tail;
    size_t gate, total;
    __host__ __device__ carve(int N, int M, const typename Iou::source& src, const typename Gate::source& gsrc = typename Gate::source()) {
        constexpr unsigned ALIGN = Iou::TAIL_ALIGN > Gate::TAIL_ALIGN ? Iou::TAIL_ALIGN : Gate::TAIL_ALIGN;
        const unsigned Np = (unsigned)((N + 3) & ~3), Mp = (unsigned)((M + 3) & ~3);
        words = (COCO ? 20 : 16) * Np + 4 * Mp;
        flags = words + Iou::word_bytes(Np, Mp);
        tail = flags + ((Np + (COCO ? Mp : 0) + ALIGN - 1) & ~(ALIGN - 1));
        gate = tail + Iou::tail_bytes(N, M, Np, Mp, src);
        if constexpr (Gate::ON) gate = (gate + 7) & ~(size_t)7;
        total = gate + Gate::bytes(Np, Mp, gsrc);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// IoU sources.  Each has: `source` (its operands in HBM, a kernel argument), its share of the LDS (word_bytes, TAIL_ALIGN,
// tail_bytes), stage() (carve that share and fill its rows) with stage_det(n) / stage_gt(m) (what rides along in the kernel's own
// loops over the detections and the ground truths: every separate loop is one more round trip to HBM; the kernel synchronises
// afterwards), the default areas in pixels for the range test - det_area(n) out of LDS after the synchronise, gt_area(m) out of
// HBM before it -, begin(d) (the per-detection set-up) and iou(m, crowd).  For a crowd region the union is the detection's own area.
// ---------------------------------------------------------------------------------------------------------------------

// boxes (x, y, w, h), normalised: box_pred [B,N,4], gt_box [B,M,4].  LDS: det boxes, gt boxes.
struct box_iou {
    struct source {
        const float* box_pred;
        const float* gt_box;
    };
    static constexpr unsigned TAIL_ALIGN = 1;
    static __host__ __device__ unsigned word_bytes(unsigned Np, unsigned Mp) { return 16 * (Np + Mp); }
    static __host__ __device__ size_t tail_bytes(int, int, size_t, size_t, const source&) { return 0; }

    const float* gt_rows;        // gt_box of this image, in HBM
    float *s_box, *g_box;
    double dx0, dy0, dx1, dy1, a_det;

    __device__ __forceinline__ void stage(const source& src, int b, int N, int M, unsigned char* words, unsigned char*, int tid, int nthr) {
        const float* det_rows = src.box_pred + (int64_t)b * N * 4;
        gt_rows = src.gt_box + (int64_t)b * M * 4;
        s_box = reinterpret_cast<float*>(words);
        g_box = s_box + 4 * ((N + 3) & ~3);
        for (int k = tid; k < 4 * N; k += nthr) s_box[k] = det_rows[k];
        for (int k = tid; k < 4 * M; k += nthr) g_box[k] = gt_rows[k];
    }
    __device__ __forceinline__ void stage_det(int) {}
    __device__ __forceinline__ void stage_gt(int) {}
    __device__ __forceinline__ double det_area(int n, double scale) const {
        const double dw = fmax((double)s_box[4 * n + 2], 0.0), dh = fmax((double)s_box[4 * n + 3], 0.0);
        return (dw * dh) * scale;
    }
    __device__ __forceinline__ double gt_area(int m, double scale) const {
        const double gw = fmax((double)gt_rows[4 * m + 2], 0.0), gh = fmax((double)gt_rows[4 * m + 3], 0.0);
        return (gw * gh) * scale;
    }
    __device__ __forceinline__ void begin(int d) {
        dx0 = (double)s_box[4 * d + 0];
        dy0 = (double)s_box[4 * d + 1];
        const double dw = fmax((double)s_box[4 * d + 2], 0.0), dh = fmax((double)s_box[4 * d + 3], 0.0);
        dx1 = dx0 + dw;
        dy1 = dy0 + dh;
        a_det = dw * dh;
    }
    __device__ __forceinline__ double iou(int m, bool crowd) const {
        const double gx0 = (double)g_box[4 * m + 0], gy0 = (double)g_box[4 * m + 1];
        const double gw = fmax((double)g_box[4 * m + 2], 0.0), gh = fmax((double)g_box[4 * m + 3], 0.0);
        const double gx1 = gx0 + gw, gy1 = gy0 + gh;
        const double a_gt = gw * gh;
        const double iw = fmax(fmin(dx1, gx1) - fmax(dx0, gx0), 0.0);
        const double ih = fmax(fmin(dy1, gy1) - fmax(dy0, gy0), 0.0);
        const double inter = iw * ih;
        const double uni = crowd ? a_det : (a_det + a_gt) - inter;
        return uni > 0.0 ? inter / uni : 0.0;
    }
};

// What the two mask sources share: the masks' set bits, det_pop [B,N] and gt_pop [B,M], staged in LDS, and the IoU as ONE IEEE
// fp64 division of two exact integers - equal rationals (2/4 and 3/6) give equal doubles and 1/2 meets the threshold 0.5: ties
// and IoUs ON a threshold are the normal case with integer pixel counts, and NumPy's count_nonzero ratio is reproduced bit for
// bit.  P is the pixels a mask has (the default areas scale the set bits by image pixels / P).
struct pixel_counts {
    static __host__ __device__ unsigned word_bytes(unsigned Np, unsigned Mp) { return 4 * (Np + Mp); }

    const int32_t *det_rows, *gt_rows;      // det_pop and gt_pop of this image, in HBM
    int *s_area, *g_area;
    int P;
    long long a_det;

    __device__ __forceinline__ void carve_counts(const int32_t* det_pop, const int32_t* gt_pop, int pixels, int b, int N, int M,
                                                 unsigned char* words) {
        det_rows = det_pop + (int64_t)b * N;
        gt_rows = gt_pop + (int64_t)b * M;
        P = pixels;
        s_area = reinterpret_cast<int*>(words);
        g_area = s_area + ((N + 3) & ~3);
    }
    __device__ __forceinline__ void stage_det(int n) { s_area[n] = det_rows[n]; }
    __device__ __forceinline__ void stage_gt(int m) { g_area[m] = gt_rows[m]; }
    __device__ __forceinline__ double det_area(int n, double scale) const { return (double)s_area[n] * scale / (double)P; }
    __device__ __forceinline__ double gt_area(int m, double scale) const { return (double)gt_rows[m] * scale / (double)P; }
    __device__ __forceinline__ double ratio(long long inter, int m, bool crowd) const {
        const long long uni = crowd ? a_det : a_det + (long long)g_area[m] - inter;
        return uni > 0 ? (double)inter / (double)uni : 0.0;
    }
};

// masks packed into 64-bit words (mask_binarize): det_bits [B,N,W], gt_bits [B,M,W].  LDS: the counts, then det words, gt words.
struct words_iou : pixel_counts {
    struct source {
        const unsigned long long* det_bits;
        const int32_t* det_pop;
        const unsigned long long* gt_bits;
        const int32_t* gt_pop;
        int P, W;                // P is not read without COCO
    };
    static constexpr unsigned TAIL_ALIGN = 8;
    static __host__ __device__ size_t tail_bytes(int, int, size_t Np, size_t Mp, const source& src) { return 8 * (size_t)src.W * (Np + Mp); }

    const unsigned long long *s_bits, *g_bits, *dw;
    int W;

    __device__ __forceinline__ void stage(const source& src, int b, int N, int M, unsigned char* words, unsigned char* tail, int tid, int nthr) {
        carve_counts(src.det_pop, src.gt_pop, src.P, b, N, M, words);
        W = src.W;
        unsigned long long* sb = reinterpret_cast<unsigned long long*>(tail);
        unsigned long long* gb = sb + (size_t)((N + 3) & ~3) * W;
        for (int k = tid; k < N * W; k += nthr) sb[k] = src.det_bits[(int64_t)b * N * W + k];
        for (int k = tid; k < M * W; k += nthr) gb[k] = src.gt_bits[(int64_t)b * M * W + k];
        s_bits = sb;
        g_bits = gb;
    }
    __device__ __forceinline__ void begin(int d) {
        dw = s_bits + (size_t)d * W;
        a_det = s_area[d];
    }
    __device__ __forceinline__ double iou(int m, bool crowd) const {
        const unsigned long long* gw = g_bits + (size_t)m * W;
        long long inter = 0;
        for (int w = 0; w < W; ++w) inter += __popcll(dw[w] & gw[w]);
        return ratio(inter, m, crowd);
    }
};

// a precomputed intersection (K21): inter [B,N,M]; pix [B] the pixels a mask of image b has.  LDS: the counts, then with STAGED
// the image's inter [N,M]; without it a lane reads its entries from HBM.
struct inter_source {
    const int32_t* inter;
    const int32_t* det_pop;
    const int32_t* gt_pop;
    const int32_t* pix;
};
template <bool STAGED>
struct inter_iou : pixel_counts {
    typedef inter_source source;
    static constexpr unsigned TAIL_ALIGN = 8;
    static __host__ __device__ size_t tail_bytes(int N, int M, size_t, size_t, const source&) { return STAGED ? 4 * (size_t)N * M : 0; }

    const int32_t *inter_b, *row_hbm;
    const int *s_inter, *row_lds;
    int M;

    __device__ __forceinline__ void stage(const source& src, int b, int N, int M_, unsigned char* words, unsigned char* tail, int tid, int nthr) {
        carve_counts(src.det_pop, src.gt_pop, src.pix[b], b, N, M_, words);
        M = M_;
        inter_b = src.inter + (int64_t)b * N * M;
        if constexpr (STAGED) {
            int* si = reinterpret_cast<int*>(tail);
            for (int k = tid; k < N * M; k += nthr) si[k] = inter_b[k];
            s_inter = si;
        }
    }
    __device__ __forceinline__ void begin(int d) {
        if constexpr (STAGED) row_lds = s_inter + (size_t)d * M;
        else row_hbm = inter_b + (int64_t)d * M;
        a_det = s_area[d];
    }
    __device__ __forceinline__ double iou(int m, bool crowd) const {
        long long in;
        if constexpr (STAGED) in = row_lds[m];
        else in = row_hbm[m];
        return ratio(in, m, crowd);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// Grid B, or (B, A) with COCO: one workgroup per image (and area range), 64 T threads: one wave per threshold.  With COCO every
// workgroup ranks its image again (N^2 compares out of LDS, cheaper than a second launch and a round trip through HBM).
// Outputs: order [B,N]; tp_bits [B,N], matched_gt [B,T,N]; gt_count [C] is added to.  With COCO also class_rank [B,N], ig_bits, and
// the per-range outputs gain a leading A: tp_bits / ig_bits [A,B,N], matched_gt [A,B,T,N], gt_count [A,C].  Without COCO gt_crowd,
// gt_area, image_hw, area_ranges, class_rank and ig_bits are not read (null).
// With a gate the grid is (B, A, F): blockIdx.z = f selects the gate's threshold, every (t, f) pair is matched on its own, and tp_bits /
// ig_bits [F,A,B,N], matched_gt [F,A,B,T,N] gain a leading F.  order, class_rank and gt_count do not depend on f: the f = 0 workgroups
// write them.
// ---------------------------------------------------------------------------------------------------------------------
template <class Iou, bool COCO, class Gate = no_gate>
__global__ __launch_bounds__(1024) void coco_match_kernel(typename Iou::source src, const float* __restrict__ score, const int32_t* __restrict__ label,
                                                          const int32_t* __restrict__ gt_label, const uint8_t* __restrict__ gt_crowd,
                                                          const float* __restrict__ gt_area, const int32_t* __restrict__ num_objects,
                                                          const int32_t* __restrict__ image_hw, const double* __restrict__ area_ranges,
                                                          match_thresholds thr, int B, int N, int M, int C, int T, int max_dets,
                                                          int32_t* __restrict__ order, int32_t* __restrict__ class_rank,
                                                          uint16_t* __restrict__ tp_bits, uint16_t* __restrict__ ig_bits,
                                                          int32_t* __restrict__ matched_gt, int32_t* __restrict__ gt_count,
                                                          typename Gate::source gsrc = typename Gate::source()) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const carve<Iou, COCO, Gate> at(N, M, src, gsrc);
    const int Np = (N + 3) & ~3;
    float* s_score = reinterpret_cast<float*>(smem);
    int* s_label = reinterpret_cast<int*>(s_score + Np);
    int* s_order = s_label + Np;
    unsigned* s_tp = reinterpret_cast<unsigned*>(s_order + Np);
    unsigned* s_ig = s_tp + Np;                                // COCO only
    int* g_label = reinterpret_cast<int*>(s_tp + (COCO ? 2 : 1) * Np);
    unsigned char* s_flag = smem + at.flags;
    unsigned char* g_flag = s_flag + Np;                       // COCO only

    const int b = blockIdx.x, a = COCO ? blockIdx.y : 0, tid = threadIdx.x, nthr = blockDim.x;
    const int gf = Gate::ON ? blockIdx.z : 0;      // the gate's threshold
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;
    const int64_t abase = ((int64_t)(Gate::ON ? gf * (int)gridDim.y + a : a) * B + b) * N;      // into tp_bits / ig_bits [A,B,N] ([F,A,B,N])
    double scale = 0.0, lo = 0.0, hi = 0.0;
    if constexpr (COCO) {
        scale = (double)image_hw[2 * b] * (double)image_hw[2 * b + 1];
        lo = area_ranges[2 * a];
        hi = area_ranges[2 * a + 1];
    }

    Iou iou;
    iou.stage(src, b, N, M, smem + at.words, smem + at.tail, tid, nthr);
    Gate gate;
    gate.stage(gsrc, gf, b, N, M, smem + at.gate, tid, nthr);
    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        if constexpr (COCO) s_ig[n] = 0u;
        s_flag[n] = 0;
        iou.stage_det(n);
    }
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        bool ignore = false;
        if constexpr (COCO) {
            unsigned char f = 0;
            if (real) {
                const bool crowd = gt_crowd[gbase + m] != 0;
                const double ar = gt_area ? (double)gt_area[gbase + m] : iou.gt_area(m, scale);
                ignore = crowd || ar < lo || ar > hi;          // both bounds inclusive
                f = (unsigned char)((ignore ? G_IGNORE : 0) | (crowd ? G_CROWD : 0));
            }
            g_flag[m] = f;
        }
        g_label[m] = real ? gl : -1;
        iou.stage_gt(m);
        if (real && !ignore && gf == 0) atomicAdd(&gt_count[(int64_t)a * C + gl], 1);
    }
    for (int64_t k = tid; k < (int64_t)T * N; k += nthr) matched_gt[abase * T + k] = -1;
    __syncthreads();

    // rank by counting: descending score, equal scores in ascending query order (a stable sort, exactly); the same pass
    // counts the detections of the query's own class that come before it (with COCO an output: the rank within the class)
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
        unsigned char f = crank < max_dets ? F_KEEP : 0;
        if constexpr (COCO) {
            const double ar = iou.det_area(n, scale);
            f |= (ar < lo || ar > hi) ? F_OUT : 0;
            if (a == 0 && gf == 0) class_rank[dbase + n] = crank;
        }
        s_flag[n] = f;
    }
    __syncthreads();
    if (a == 0 && gf == 0)
        for (int n = tid; n < N; n += nthr) order[dbase + n] = s_order[n];

    const int wave = tid >> 6, lane = tid & 63;
    if (wave < T) {
        const double th = fmin(thr.v[wave], 1.0 - 1e-10);
        int32_t* mrow = matched_gt + (abase * T + (int64_t)wave * N);
        unsigned taken = 0u;                     // bit k: ground truth lane + 64 k is consumed at this threshold (a lane owns its own)
        for (int r = 0; r < N; ++r) {
            const int d = s_order[r];
            if (d < 0 || !(s_flag[d] & F_KEEP)) continue;   // wave-uniform
            const int dl = s_label[d];
            iou.begin(d);
            gate.begin(d);
            // phase 0: the non-ignored ground truths; phase 1 (COCO), only when phase 0 found none: the ignored ones (COCOeval sorts
            // the ignored ground truths last and breaks out of its scan on reaching them with a match in hand).  `phase` and `bestm`
            // after the butterfly are the same in every lane, so the whole wave takes the same path into each reduction.
            double best = -1.0;
            int bestm = -1;
            for (int phase = 0; phase < (COCO ? 2 : 1) && bestm < 0; ++phase) {
                best = -1.0;
                for (int k = 0, m = lane; m < M; m += 64, ++k) {
                    if (g_label[m] != dl) continue;
                    bool crowd = false;
                    if constexpr (COCO) {
                        const unsigned f = g_flag[m];
                        if ((int)(f & G_IGNORE) != phase) continue;
                        crowd = (f & G_CROWD) != 0;
                    }
                    if (((taken >> k) & 1u) && !crowd) continue;
                    const double v = iou.iou(m, crowd);
                    if (v >= th && v >= best && gate.pass(m)) { best = v; bestm = m; }      // ascending m: on equal IoU the larger index stays
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
                    bool ignored = false;
                    if constexpr (COCO) ignored = (g_flag[bestm] & G_IGNORE) != 0;
                    if (ignored) atomicOr(&s_ig[d], 1u << wave);
                    else atomicOr(&s_tp[d], 1u << wave);
                }
            } else if (COCO && lane == 0 && (s_flag[d] & F_OUT)) {
                atomicOr(&s_ig[d], 1u << wave);
            }
        }
    }
    __syncthreads();
    for (int n = tid; n < N; n += nthr) {
        tp_bits[abase + n] = (uint16_t)(s_tp[n] | ((s_flag[n] & F_KEEP) ? KEEP_BIT : 0u));
        if constexpr (COCO) ig_bits[abase + n] = (uint16_t)s_ig[n];
    }
}

}  // namespace cocomatch
