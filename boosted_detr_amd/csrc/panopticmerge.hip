// panopticmerge.hip - panoptic merge and panoptic quality on gfx950 (K23-K26, include/bdetr.h): which queries become segments, the
// per-pixel merge of the kept queries' upsampled logits into one id per pixel (and pairwise disjoint bitmasks), the ground truth
// as a panoptic map, and panopticapi's matching in integers.  evaluation.PanopticEvaluator chains them with K20 and K21.
//
// Masks use maskimage.hip's layout: uint64 [Hm, Wm], pixel (x, y) is bit x mod 64 of word [y, x div 64]; bits outside the image
// are zero and are WRITTEN as zero here.
//
// Compiled with -ffp-contract=off like maskimage.hip: K24's value of a pixel is K19's - both call mask_upsample.h (no FMA) -, so
// the merged masks of a single kept query are K19's bit for bit and NumPy reproduces the winner of every pixel.
#include "mask_upsample.h"
#include <limits.h>

using namespace maskup;

namespace {

typedef unsigned long long u64;

constexpr int PM_THREADS = 256;
constexpr int PM_MAX_DIM = 4096;          // image extents (K19's limit)
constexpr int PM_MAX_N = 1024;            // queries per image (K21's limit)
constexpr int PM_MAX_M = 1024;            // ground-truth rows per image (K21's limit)
constexpr int PM_MAX_C = 65536;           // classes
constexpr size_t PM_LDS_LIMIT = 64 * 1024;      // the default dynamic LDS of a workgroup

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// K23: score, label [B,N] -> seg_of [B,N].  One workgroup per image.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void panoptic_select_kernel(const float* __restrict__ score, const int32_t* __restrict__ label,
                                                                     const uint8_t* __restrict__ is_stuff, int N, int C, float threshold,
                                                                     int32_t* __restrict__ seg_of) {
    __shared__ int s_label[PM_MAX_N];
    __shared__ unsigned char s_kept[PM_MAX_N];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t base = (int64_t)b * N;
    for (int n = tid; n < N; n += PM_THREADS) {
        s_label[n] = label[base + n];
        s_kept[n] = score[base + n] > threshold ? 1 : 0;       // NaN > t is false
    }
    __syncthreads();
    for (int n = tid; n < N; n += PM_THREADS) {
        int s = -1;
        if (s_kept[n]) {
            s = n;
            const int l = s_label[n];
            if (is_stuff && l >= 0 && l < C && is_stuff[l]) {
                for (int j = 0; j < n; ++j)
                    if (s_kept[j] && s_label[j] == l) {
                        s = j;
                        break;
                    }
            }
        }
        seg_of[base + n] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K24: logits [B,N,G,G], seg_of [B,N] -> ids [B,Hm,64 Wm], bits [B,N,Hm,Wm] (optional), pop [B,N]
// ---------------------------------------------------------------------------------------------------------------------
// Grid (groups of runs, B).  A wave owns one run of 64 consecutive words of its image's Hm x Wm, as in K19: per word, lane l
// evaluates pixel x = 64 wd + l.  The workgroup first compacts its image's kept queries (seg_of in [0, N)) in ascending order
// into LDS - a query that is not kept costs nothing per pixel - and each lane then walks the kept list with a running
// (best value, best position): v > best with best starting at 0 keeps the lowest index on a tie, needs v > 0 and never takes a
// NaN.  The kept queries' logits are NOT staged: 100 kept queries at G = 23 are 211 KB, more than a CU's LDS, and a chunked
// staging would need the running best of 64 words per lane; the four logits a pixel needs are read through L1 / L2 instead (the
// 64 lanes of a word touch a few neighbouring cells of two grid rows).
// The run's ids stay in LDS as int16 [64 words][64 lanes] - the output's own order, stored with 16-byte stores - and every
// segment's words are ballots over them: lane k keeps word k, one coalesced 512-byte store per (row, run).  Rows that are no
// segment id are stored as zeros.
// LDS (dynamic): x weights double [64 Wm], x cell pairs uint16 [64 Wm] (ia | ib << 8), ids int16 [waves][4096], kept int16 [N],
// their seg_of int16 [N].
__global__ __launch_bounds__(PM_THREADS) void panoptic_merge_kernel(const float* __restrict__ logits, const int32_t* __restrict__ seg_of,
                                                                    const int32_t* __restrict__ image_hw, int N, int G, int Hm, int Wm,
                                                                    int16_t* __restrict__ ids, u64* __restrict__ bits,
                                                                    int32_t* __restrict__ pop) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ u64 s_segmask[PM_MAX_N / 64];
    __shared__ int s_wcnt[PM_THREADS / 64];
    const int Wx = Wm * 64, GG = G * G, tid = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
    double* s_tx = reinterpret_cast<double*>(smem);
    uint16_t* s_ix = reinterpret_cast<uint16_t*>(s_tx + Wx);
    int16_t* s_id = reinterpret_cast<int16_t*>(s_ix + Wx);
    int16_t* s_kept = s_id + nw * 4096;
    int16_t* s_seg = s_kept + N;

    const int b = blockIdx.y, wave = tid >> 6, lane = tid & 63;
    const int h = min(max(image_hw[2 * b], 0), Hm), w = min(max(image_hw[2 * b + 1], 0), Wx);      // never past the buffers
    const int32_t* so = seg_of + (int64_t)b * N;

    for (int k = tid; k < PM_MAX_N / 64; k += nthr) s_segmask[k] = 0ull;
    for (int x = tid; x < w; x += nthr) {
        const axis a = axis_rule(x, w, G);
        s_tx[x] = a.t;
        s_ix[x] = (uint16_t)(a.ia | (a.ib << 8));
    }
    __syncthreads();
    // ordered compaction: a ballot per wave, the waves' counts through LDS
    int K = 0;                                                   // the same in every thread
    for (int n0 = 0; n0 < N; n0 += nthr) {
        const int n = n0 + tid;
        const int s = n < N ? so[n] : -1;
        const bool kept = s >= 0 && s < N;
        const u64 m = __ballot(kept);
        if (lane == 0) s_wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = K;
        for (int v = 0; v < nw; ++v) {
            if (v < wave) off += s_wcnt[v];
            K += s_wcnt[v];
        }
        if (kept) {
            const int pos = off + __popcll(m & ((1ull << lane) - 1ull));      // pos < N
            s_kept[pos] = (int16_t)n;
            s_seg[pos] = (int16_t)s;
            atomicOr(&s_segmask[s >> 6], 1ull << (s & 63));
        }
        __syncthreads();
    }

    const int total = Hm * Wm;                                   // <= 4096 * 64
    const int first = (blockIdx.x * nw + wave) * 64;
    const int cnt = min(64, max(total - first, 0));              // trailing waves of the last group own nothing
    int16_t* my_id = s_id + wave * 4096;
    const float* Lb = logits + (int64_t)b * N * GG;
    {
        int y = first / Wm, wd = first - y * Wm;
        int cur_y = -1, oa = 0, ob = 0;
        double ty = 0.0, uy = 1.0;
        for (int k = 0; k < cnt; ++k) {
            int id = -1;
            if (y < h && wd * 64 < w) {
                if (y != cur_y) {
                    const axis a = axis_rule(y, h, G);
                    oa = a.ia * G;
                    ob = a.ib * G;
                    ty = a.t;
                    uy = 1.0 - ty;
                    cur_y = y;
                }
                const int x = wd * 64 + lane;
                if (x < w) {
                    const int ix = s_ix[x], xa = ix & 255, xb = ix >> 8;
                    const double tx = s_tx[x], ux = 1.0 - tx;
                    const int a0 = oa + xa, a1 = oa + xb, b0 = ob + xa, b1 = ob + xb;      // all < G G
                    double best = 0.0;
                    int bq = -1;
                    for (int q = 0; q < K; ++q) {
                        const float* L = Lb + (int)s_kept[q] * GG;
                        const double v = bilinear(ux, tx, uy, ty, L[a0], L[a1], L[b0], L[b1]);
                        if (v > best) {                          // NaN > best is false; a tie keeps the lower query
                            best = v;
                            bq = q;
                        }
                    }
                    if (bq >= 0) id = s_seg[bq];
                }
            }
            my_id[k * 64 + lane] = (int16_t)id;
            if (++wd == Wm) {
                wd = 0;
                ++y;
            }
        }
    }
    __syncthreads();
    if (cnt > 0) {
        const uint4* src = reinterpret_cast<const uint4*>(my_id);
        uint4* dst = reinterpret_cast<uint4*>(ids + ((int64_t)b * total + first) * 64);
        for (int v = lane; v < cnt * 8; v += 64) dst[v] = src[v];
        for (int n = 0; n < N; ++n) {
            const bool is_seg = ((s_segmask[n >> 6] >> (n & 63)) & 1ull) != 0;      // the same in every lane
            u64 mine = 0ull;
            if (is_seg) {
                int c = 0;
                for (int k = 0; k < cnt; ++k) {
                    const u64 word = __ballot((int)my_id[k * 64 + lane] == n);
                    c += __popcll(word);
                    if (k == lane) mine = word;
                }
                if (lane == 0 && c) atomicAdd(&pop[(int64_t)b * N + n], c);
            }
            if (bits && lane < cnt) bits[((int64_t)b * N + n) * total + first + lane] = mine;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K25: gt_bits [B,M,Hm,Wm] in place -> exclusive; gt_pop [B,M].  Grid (word groups, B): a lane owns one word position of every row.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void panoptic_gt_exclusive_kernel(u64* __restrict__ bits, const int32_t* __restrict__ gt_label,
                                                                           const int32_t* __restrict__ num_objects, int M, int C, int total,
                                                                           int32_t* __restrict__ gt_pop) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int wpos = blockIdx.x * PM_THREADS + threadIdx.x;
    const bool valid = wpos < total;
    const int n_obj = max(0, min(num_objects[b], M));
    u64* p = bits + (int64_t)b * M * total + wpos;
    const int32_t* gl = gt_label + (int64_t)b * M;
    u64 seen = 0ull;
    for (int m = 0; m < M; ++m) {
        const int l = gl[m];
        const bool seg = m < n_obj && l >= 2 && l < C;            // uniform over the workgroup
        if (seg) {
            u64 in = 0ull, out = 0ull;
            if (valid) {
                in = p[(int64_t)m * total];
                out = in & ~seen;
                seen |= in;
                if (out != in) p[(int64_t)m * total] = out;
            }
            const int c = wave_sum_int(__popcll(out));
            if (lane == 0 && c) atomicAdd(&gt_pop[(int64_t)b * M + m], c);
        } else if (valid) {
            p[(int64_t)m * total] = 0ull;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K26: panopticapi's pq_compute_single_core in integers.  One workgroup per image.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PM_THREADS) void panoptic_match_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ pred_pop,
                                                                    const int32_t* __restrict__ pred_label, const int32_t* __restrict__ seg_of,
                                                                    const int32_t* __restrict__ gt_pop, const int32_t* __restrict__ gt_label,
                                                                    const uint8_t* __restrict__ gt_crowd, const int32_t* __restrict__ num_objects,
                                                                    int N, int M, int C, int min_area, int32_t* __restrict__ gt_state,
                                                                    int32_t* __restrict__ pred_state, int32_t* __restrict__ match_inter,
                                                                    int32_t* __restrict__ match_union) {
    __shared__ long long s_void[PM_MAX_N];
    __shared__ int s_plabel[PM_MAX_N];        // the predicted segment's label, or INT_MIN: not a segment
    __shared__ int s_ppop[PM_MAX_N];
    __shared__ int s_glabel[PM_MAX_M];        // the ground-truth segment's label, or -1: not a segment
    __shared__ int s_gpop[PM_MAX_M];
    __shared__ unsigned char s_gcrowd[PM_MAX_M];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t nb = (int64_t)b * N, mb = (int64_t)b * M;
    const int32_t* in_b = inter + nb * M;
    const int n_obj = max(0, min(num_objects[b], M));
    const int need = max(min_area, 1);

    for (int m = tid; m < M; m += PM_THREADS) {
        const int l = gt_label[mb + m], gp = gt_pop[mb + m];
        const bool seg = m < n_obj && l >= 2 && l < C && gp >= 1;
        s_glabel[m] = seg ? l : -1;
        s_gpop[m] = gp;
        s_gcrowd[m] = (seg && gt_crowd && gt_crowd[mb + m]) ? 1 : 0;
    }
    for (int n = tid; n < N; n += PM_THREADS) {
        const int pp = pred_pop[nb + n];
        const bool seg = seg_of[nb + n] == n && pp >= need;
        long long sum = 0;
        for (int m = 0; m < M; ++m) sum += in_b[(int64_t)n * M + m];
        s_plabel[n] = seg ? pred_label[nb + n] : INT_MIN;
        s_ppop[n] = pp;
        s_void[n] = (long long)pp - sum;
    }
    __syncthreads();

    // the match test in integers: union = pred_pop + gt_pop - inter - void_n; 2 inter > union  (IoU > 1/2)
    for (int n = tid; n < N; n += PM_THREADS) {
        int st = -3;
        const int pl = s_plabel[n];
        if (pl != INT_MIN) {
            st = -1;
            const long long pp = s_ppop[n], vd = s_void[n];
            long long crowd = 0;
            for (int m = 0; m < M; ++m) {
                if (s_glabel[m] < 0 || s_glabel[m] != pl) continue;
                const long long in = in_b[(int64_t)n * M + m];
                if (s_gcrowd[m]) {
                    crowd += in;
                    continue;
                }
                const long long uni = pp + (long long)s_gpop[m] - in - vd;
                if (st < 0 && 2 * in > uni) st = m;              // at most one m can hold on disjoint maps: the lowest otherwise
            }
            if (st < 0 && 2 * (vd + crowd) > pp) st = -2;
        }
        pred_state[nb + n] = st;
    }
    for (int m = tid; m < M; m += PM_THREADS) {
        int st = -3, mi = 0, mu = 0;
        const int l = s_glabel[m];
        if (l >= 0 && s_gcrowd[m]) {
            st = -2;
        } else if (l >= 0) {
            st = -1;
            const long long gp = s_gpop[m];
            for (int n = 0; n < N && st < 0; ++n) {
                if (s_plabel[n] != l) continue;
                const long long in = in_b[(int64_t)n * M + m];
                const long long uni = (long long)s_ppop[n] + gp - in - s_void[n];
                if (2 * in > uni) {
                    st = n;
                    mi = (int)in;
                    mu = (int)uni;
                }
            }
        }
        gt_state[mb + m] = st;
        match_inter[mb + m] = mi;
        match_union[mb + m] = mu;
    }
}

bool pm_layout_ok(int Hm, int Wm) { return Hm >= 1 && Hm <= PM_MAX_DIM && Wm >= 1 && Wm <= PM_MAX_DIM / 64; }

}  // namespace

extern "C" int bdetr_panoptic_select(const float* score, const int32_t* label, const uint8_t* is_stuff, int B, int N, int C, float threshold,
                                     int32_t* seg_of, void* stream) {
    BDETR_CHECK_ARG(score && label && seg_of, "bdetr_panoptic_select: null pointer (only is_stuff may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= PM_MAX_N && C >= 3 && C <= PM_MAX_C,
                    "bdetr_panoptic_select: bad sizes B=%d N=%d C=%d (limits: B in [1, 65535], N in [1, %d], C in [3, %d])", B, N, C, PM_MAX_N,
                    PM_MAX_C);
    BDETR_CHECK_ARG(threshold >= 0.0f && threshold < 1.0f, "bdetr_panoptic_select: threshold must be in [0, 1), got %g", (double)threshold);
    hipLaunchKernelGGL(panoptic_select_kernel, dim3((unsigned)B), dim3(PM_THREADS), 0, (hipStream_t)stream, score, label, is_stuff, N, C,
                       threshold, seg_of);
    return bdetr_launch_status("panoptic_select");
}

extern "C" int bdetr_panoptic_merge(const float* logits, const int32_t* seg_of, const int32_t* image_hw, int B, int N, int G, int Hm, int Wm,
                                    int16_t* ids, uint64_t* bits, int32_t* pop, void* stream) {
    BDETR_CHECK_ARG(logits && seg_of && image_hw && ids && pop, "bdetr_panoptic_merge: null pointer (only bits may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= PM_MAX_N && G >= 1 && G <= MAX_G && pm_layout_ok(Hm, Wm),
                    "bdetr_panoptic_merge: bad sizes B=%d N=%d G=%d Hm=%d Wm=%d (limits: B in [1, 65535], N in [1, %d], G in [1, %d], "
                    "Hm in [1, %d], Wm in [1, %d])", B, N, G, Hm, Wm, PM_MAX_N, MAX_G, PM_MAX_DIM, PM_MAX_DIM / 64);
    BDETR_CHECK_ARG((uintptr_t)ids % 16 == 0, "bdetr_panoptic_merge: ids must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = bdetr_zero_bytes(pop, (size_t)B * N * sizeof(int32_t), st)) return e;      // the waves ADD into it
    // the x tables, the kept list and 8 KiB of ids per wave: as many waves (4, 2, 1) as the default 64 KiB hold
    const size_t fixed = (size_t)Wm * 64 * 10 + (size_t)N * 4;
    int waves = PM_THREADS / 64;
    while (waves > 1 && fixed + (size_t)waves * 8192 > PM_LDS_LIMIT) waves >>= 1;
    const size_t lds = fixed + (size_t)waves * 8192;                                        // 4 waves up to Wm = 50 at N = 100, else 2
    const int runs = (Hm * Wm + 63) / 64;
    hipLaunchKernelGGL(panoptic_merge_kernel, dim3((unsigned)((runs + waves - 1) / waves), (unsigned)B), dim3(64 * waves), lds, st, logits,
                       seg_of, image_hw, N, G, Hm, Wm, ids, reinterpret_cast<u64*>(bits), pop);
    return bdetr_launch_status("panoptic_merge");
}

extern "C" int bdetr_panoptic_gt_exclusive(uint64_t* gt_bits, const int32_t* gt_label, const int32_t* num_objects, int B, int M, int C, int Hm,
                                           int Wm, int32_t* gt_pop, void* stream) {
    BDETR_CHECK_ARG(gt_bits && gt_label && num_objects && gt_pop, "bdetr_panoptic_gt_exclusive: null pointer");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && M > 0 && M <= PM_MAX_M && C >= 3 && C <= PM_MAX_C && pm_layout_ok(Hm, Wm),
                    "bdetr_panoptic_gt_exclusive: bad sizes B=%d M=%d C=%d Hm=%d Wm=%d (limits: B in [1, 65535], M in [1, %d], C in [3, %d], "
                    "Hm in [1, %d], Wm in [1, %d])", B, M, C, Hm, Wm, PM_MAX_M, PM_MAX_C, PM_MAX_DIM, PM_MAX_DIM / 64);
    hipStream_t st = (hipStream_t)stream;
    if (int e = bdetr_zero_bytes(gt_pop, (size_t)B * M * sizeof(int32_t), st)) return e;   // the waves ADD into it
    const int total = Hm * Wm;
    hipLaunchKernelGGL(panoptic_gt_exclusive_kernel, dim3((unsigned)((total + PM_THREADS - 1) / PM_THREADS), (unsigned)B), dim3(PM_THREADS), 0,
                       st, reinterpret_cast<u64*>(gt_bits), gt_label, num_objects, M, C, total, gt_pop);
    return bdetr_launch_status("panoptic_gt_exclusive");
}

extern "C" int bdetr_panoptic_match(const int32_t* inter, const int32_t* pred_pop, const int32_t* pred_label, const int32_t* seg_of,
                                    const int32_t* gt_pop, const int32_t* gt_label, const uint8_t* gt_crowd, const int32_t* num_objects, int B,
                                    int N, int M, int C, int min_area, int32_t* gt_state, int32_t* pred_state, int32_t* match_inter,
                                    int32_t* match_union, void* stream) {
    BDETR_CHECK_ARG(inter && pred_pop && pred_label && seg_of && gt_pop && gt_label && num_objects && gt_state && pred_state && match_inter &&
                    match_union, "bdetr_panoptic_match: null pointer (only gt_crowd may be null)");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= PM_MAX_N && M > 0 && M <= PM_MAX_M && C >= 3 && C <= PM_MAX_C && min_area >= 0,
                    "bdetr_panoptic_match: bad sizes B=%d N=%d M=%d C=%d min_area=%d (limits: B in [1, 65535], N in [1, %d], M in [1, %d], "
                    "C in [3, %d], min_area >= 0)", B, N, M, C, min_area, PM_MAX_N, PM_MAX_M, PM_MAX_C);
    hipLaunchKernelGGL(panoptic_match_kernel, dim3((unsigned)B), dim3(PM_THREADS), 0, (hipStream_t)stream, inter, pred_pop, pred_label, seg_of,
                       gt_pop, gt_label, gt_crowd, num_objects, N, M, C, min_area, gt_state, pred_state, match_inter, match_union);
    return bdetr_launch_status("panoptic_match");
}
