// maskimage.hip - mask AP at image resolution on gfx950 (K19-K22, include/bdetr.h): the query masks upsampled to the image
// (bilinear on the logits, cut at 0), the ground truths' exact source bitmasks, the popcount intersection of the two, and COCOeval's
// matching fed from that intersection.  evaluation.CocoImageMaskEvaluator chains the four.
//
// One layout for every mask of a batch: uint64 [Hm, Wm], Hm = max height, Wm = ceil(max width / 64), pixel (x, y) is bit x mod 64 of
// word [y, x div 64]; bits at x >= w_b and rows y >= h_b are zero and are WRITTEN as zero by K19 and K20 (no memset is relied on).
//
// Compiled with -ffp-contract=off like maskmetric.hip: K19's fp64 interpolation rounds every product and every sum on its own (no
// FMA), so NumPy reproduces it bit for bit, and K22's IoU stays one IEEE division of two exact integers.
#include "common.h"
#include <limits.h>

namespace {

typedef unsigned long long u64;

constexpr int MI_THREADS = 256;
constexpr int MI_MAX_G = 32;              // logit grid cells per side (K18's limit)
constexpr int MI_MAX_DIM = 4096;          // image extents (K18's limit)
constexpr int MI_COORD = 1 << 23;         // |snapped coordinate| (1/256 pixel)
constexpr int MI_BAND_WORDS = 3072;       // 64-bit words per LDS band buffer (two buffers: 48 KiB), as maskraster.hip
constexpr int MI_KIND_POLY = 1, MI_KIND_RLE = 2;

// ---------------------------------------------------------------------------------------------------------------------
// K19: logits [B,N,G,G] -> bits [B,N,Hm,Wm], pop [B,N]
// ---------------------------------------------------------------------------------------------------------------------
struct mi_axis {
    int ia, ib;
    double t;
};

// target pixel p of n along an axis of G source cells: the two source cells and the weight of the second one
__device__ __forceinline__ mi_axis axis_rule(int p, int n, int G) {
    const int num = (2 * p + 1) * G - n, D = 2 * n;
    const int i0 = num >= 0 ? num / D : -((D - 1 - num) / D);      // floor division: -1 for every negative num (|num| < D)
    const int r = num - i0 * D;
    mi_axis a;
    a.ia = min(max(i0, 0), G - 1);
    a.ib = min(max(i0 + 1, 0), G - 1);
    a.t = (double)r / (double)D;
    return a;
}

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
        const mi_axis a = axis_rule(x, w, G);
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
                    const mi_axis a = axis_rule(y, h, G);
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
                    const double top = ux * (double)r0[xa] + tx * (double)r0[xb];
                    const double bot = ux * (double)r1[xa] + tx * (double)r1[xb];
                    const double v = uy * top + ty * bot;
                    on = v > 0.0;                                // NaN > 0 is false
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
// K20: the segments pack -> bits [B,M,Hm,Wm], pop [B,M].  The band code is maskraster.hip's (K18's source mask, the same
// rule): there the band is folded into grid cells and dropped, here it is stored.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long ceil_div(long long a, long long b) {      // b > 0
    long long q = a / b;
    return (a % b > 0) ? q + 1 : q;
}
__device__ __forceinline__ int clamp_coord(int v) { return min(max(v, -MI_COORD), MI_COORD); }

__global__ __launch_bounds__(MI_THREADS) void mask_source_bits_kernel(const int32_t* __restrict__ items, long long n_items,
                                                                      const int32_t* __restrict__ item_off, const int32_t* __restrict__ kind,
                                                                      const int32_t* __restrict__ hw, int Hm, int Wm, u64* __restrict__ bits,
                                                                      int32_t* __restrict__ pop) {
    __shared__ u64 s_tog[MI_BAND_WORDS];
    __shared__ u64 s_uni[MI_BAND_WORDS];
    __shared__ int s_area, s_ymin, s_ymax;

    const int o = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        s_area = 0;
        s_ymin = INT_MAX;
        s_ymax = INT_MIN;
    }
    // everything below is uniform over the workgroup: every lane reads the same descriptors
    const int kd = kind[o], h = hw[2 * o], w = hw[2 * o + 1];
    const long long off0 = item_off[o], off1 = item_off[o + 1];
    bool ok = (kd == MI_KIND_POLY || kd == MI_KIND_RLE) && h >= 1 && h <= min(MI_MAX_DIM, Hm) && w >= 1 && w <= MI_MAX_DIM &&
              ((w + 63) >> 6) <= Wm;
    ok = ok && off0 >= 0 && off0 <= off1 && off1 <= n_items;
    const int32_t* it = items + off0;
    const long long n = off1 - off0;
    const int total = Hm * Wm;
    u64* out = bits + (int64_t)o * total;
    __syncthreads();

    // the rows that can hold a set bit: [row_lo, row_hi]
    int row_lo = 0, row_hi = -1;
    long long R = 0, V = 0;
    const int32_t *ring = nullptr, *vert = nullptr;
    if (ok && kd == MI_KIND_RLE) {
        row_hi = h - 1;
    } else if (ok && kd == MI_KIND_POLY && n >= 2) {
        // items: R, ring offsets e[0..R] in vertices (e[0] = 0, e[R] = V), then V snapped (x, y) pairs
        R = it[0];
        bool pok = R >= 0 && R + 2 <= n;
        if (pok) {
            V = it[1 + R];
            pok = V >= 0 && 2 + R + 2 * V <= n;
        }
        if (pok && R > 0 && V > 0) {
            ring = it + 1;
            vert = it + 2 + R;
            for (long long v = tid; v < V; v += MI_THREADS) {
                const int y = clamp_coord(vert[2 * v + 1]);
                atomicMin(&s_ymin, y);
                atomicMax(&s_ymax, y);
            }
            __syncthreads();
            // rows whose centre 256 y + 128 lies in [ymin, ymax): no other row is crossed by any edge
            row_lo = max(0, (int)ceil_div((long long)s_ymin - 128, 256));
            row_hi = min(h - 1, (int)ceil_div((long long)s_ymax - 128, 256) - 1);
        }
    }
    if (row_hi < row_lo) {
        row_lo = 0;
        row_hi = -1;
    }
    for (int k = tid; k < row_lo * Wm; k += MI_THREADS) out[k] = 0ull;
    for (int k = (row_hi + 1) * Wm + tid; k < total; k += MI_THREADS) out[k] = 0ull;

    if (row_hi >= row_lo) {
        const int wpr = (w + 63) >> 6;
        const int band = MI_BAND_WORDS / wpr;                                       // >= 48 rows
        const u64 tail = (w & 63) ? ((1ull << (w & 63)) - 1) : ~0ull;
        int my_area = 0;
        for (int yb0 = row_lo; yb0 <= row_hi; yb0 += band) {
            const int rows = min(band, row_hi - yb0 + 1);
            for (int k = tid; k < rows * wpr; k += MI_THREADS) {
                s_tog[k] = 0ull;
                s_uni[k] = 0ull;
            }
            __syncthreads();
            if (kd == MI_KIND_RLE) {
                // items: (start, length) of the one-runs in column-major pixel order.  16 lanes per run: per column of the run,
                // the lanes set the run's rows inside the band
                const int hwpix = h * w;                                            // <= 2^24
                const int sub = tid & 15;
                for (long long r = tid >> 4; r < n / 2; r += MI_THREADS / 16) {
                    long long s = it[2 * r], e = s + (long long)it[2 * r + 1];
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
                for (long long r = 0; r < R; ++r) {
                    const long long va = min(max((long long)ring[r], 0ll), V), vb = min(max((long long)ring[r + 1], 0ll), V);
                    const int nv = (int)(vb - va);
                    if (nv < 3) continue;                                           // uniform
                    const int32_t* rv = vert + 2 * va;
                    const int sub = tid & 3;
                    for (int e = tid >> 2; e < nv; e += MI_THREADS / 4) {
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
                    for (int rr = tid; rr < rows; rr += MI_THREADS) {
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

// ---------------------------------------------------------------------------------------------------------------------
// K22: mask_match_coco_kernel (maskmetric.hip, K17) with the IoU source replaced: inter comes from K21, the pixel counts from
// K19 / K20, the masks' pixel count per image from pix.  The ranking, flags and matching loop are K17's, operation for operation.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int MSK_MAX_N = 1024;      // queries per image
constexpr int MSK_MAX_M = 1024;      // ground-truth rows per image (16 matched bits per lane)
constexpr int MSK_MAX_C = 65536;     // classes
constexpr int MSK_MAX_T = 15;        // thresholds: bits 0..14 of tp_bits, bit 15 = keep
constexpr int MSK_MAX_A = 4;         // area ranges
constexpr unsigned MSK_KEEP_BIT = 0x8000u;
constexpr size_t MSK_LDS_LIMIT = 64 * 1024;      // the default dynamic LDS of a workgroup (no opt-in to the CU's 160 KiB)
constexpr unsigned char MSK_F_KEEP = 1, MSK_F_OUT = 2;       // detection flags: kept; own area outside the range
constexpr unsigned char MSK_G_IGNORE = 1, MSK_G_CROWD = 2;   // ground-truth flags: ignored in the range; crowd (reusable)

struct mask_thresholds { double v[MSK_MAX_T + 1]; };

// Grid (B, A): one workgroup per image and area range, one wave per threshold.
// LDS (dynamic; N and M rounded up to 4): scores, labels, order, tp words, ig words, det pixel counts, gt labels, gt pixel counts,
// det flag bytes and gt flag bytes (together rounded up to 8), then with STAGED the image's inter [N,M].
template <bool STAGED>
__global__ __launch_bounds__(1024) void mask_match_coco_inter_kernel(const float* __restrict__ score, const int32_t* __restrict__ label,
                                                                     const int32_t* __restrict__ inter, const int32_t* __restrict__ det_pop,
                                                                     const int32_t* __restrict__ gt_label, const int32_t* __restrict__ gt_pop,
                                                                     const uint8_t* __restrict__ gt_crowd, const float* __restrict__ gt_area,
                                                                     const int32_t* __restrict__ num_objects, const int32_t* __restrict__ image_hw,
                                                                     const int32_t* __restrict__ pix, const double* __restrict__ area_ranges,
                                                                     mask_thresholds thr, int B, int N, int M, int C, int T, int max_dets,
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
    int* s_inter = reinterpret_cast<int*>(s_flag + ((Np + Mp + 7) & ~7));

    const int b = blockIdx.x, a = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int n_obj = max(0, min(num_objects[b], M));
    const int64_t dbase = (int64_t)b * N, gbase = (int64_t)b * M;
    const int64_t abase = ((int64_t)a * B + b) * N;            // into tp_bits / ig_bits [A,B,N]
    const double scale = (double)image_hw[2 * b] * (double)image_hw[2 * b + 1];
    const int P = pix[b];
    const double lo = area_ranges[2 * a], hi = area_ranges[2 * a + 1];
    const int32_t* inter_b = inter + dbase * M;

    for (int n = tid; n < N; n += nthr) {
        s_score[n] = score[dbase + n];
        s_label[n] = label[dbase + n];
        s_area[n] = det_pop[dbase + n];
        s_order[n] = -1;
        s_tp[n] = 0u;
        s_ig[n] = 0u;
        s_flag[n] = 0;
    }
    if (STAGED)
        for (int k = tid; k < N * M; k += nthr) s_inter[k] = inter_b[k];
    for (int m = tid; m < M; m += nthr) {
        const int gl = gt_label[gbase + m];
        const bool real = m < n_obj && gl >= 2 && gl < C;      // rows past num_objects are padding; <PAD> / <OOV> rows are ignored
        const int gp = gt_pop[gbase + m];
        unsigned char f = 0;
        if (real) {
            const bool crowd = gt_crowd[gbase + m] != 0;
            const double ar = gt_area ? (double)gt_area[gbase + m] : (double)gp * scale / (double)P;
            const bool ignore = crowd || ar < lo || ar > hi;   // both bounds inclusive
            f = (unsigned char)((ignore ? MSK_G_IGNORE : 0) | (crowd ? MSK_G_CROWD : 0));
            if (!ignore) atomicAdd(&gt_count[(int64_t)a * C + gl], 1);
        }
        g_label[m] = real ? gl : -1;
        g_area[m] = gp;
        g_flag[m] = f;
    }
    for (int64_t k = tid; k < (int64_t)T * N; k += nthr) matched_gt[abase * T + k] = -1;
    __syncthreads();

    // rank by counting, as mask_match_coco_kernel does
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
            const int32_t* irow = STAGED ? s_inter + (size_t)d * M : inter_b + (int64_t)d * M;
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
                    const long long in = irow[m];
                    const long long uni = crowd ? a_det : a_det + (long long)g_area[m] - in;
                    const double iou = uni > 0 ? (double)in / (double)uni : 0.0;
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

bool mask_layout_ok(int Hm, int Wm) { return Hm >= 1 && Hm <= MI_MAX_DIM && Wm >= 1 && Wm <= MI_MAX_DIM / 64; }

}  // namespace

extern "C" int bdetr_mask_upsample_bits(const float* logits, const int32_t* image_hw, int B, int N, int G, int Hm, int Wm, uint64_t* bits,
                                        int32_t* pop, void* stream) {
    BDETR_CHECK_ARG(logits && image_hw && bits && pop, "bdetr_mask_upsample_bits: null pointer");
    BDETR_CHECK_ARG(B > 0 && N > 0 && (int64_t)B * N <= (1 << 24) && G >= 1 && G <= MI_MAX_G && mask_layout_ok(Hm, Wm),
                    "bdetr_mask_upsample_bits: bad sizes B=%d N=%d G=%d Hm=%d Wm=%d (limits: B, N >= 1, B N <= 2^24, G in [1, %d], Hm in [1, %d], "
                    "Wm in [1, %d])", B, N, G, Hm, Wm, MI_MAX_G, MI_MAX_DIM, MI_MAX_DIM / 64);
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
                    "Wm in [1, %d], n_items in [0, 2^31))", B, M, Hm, Wm, (long long)n_items, MI_MAX_DIM, MI_MAX_DIM / 64);
    hipLaunchKernelGGL(mask_source_bits_kernel, dim3((unsigned)(B * M)), dim3(MI_THREADS), 0, (hipStream_t)stream, items, (long long)n_items,
                       item_off, kind, hw, Hm, Wm, reinterpret_cast<u64*>(bits), pop);
    return bdetr_launch_status("mask_source_bits");
}

extern "C" int bdetr_mask_inter(const uint64_t* det_bits, const uint64_t* gt_bits, const int32_t* num_objects, int B, int N, int M, int Hm,
                                int Wm, int32_t* inter, void* stream) {
    BDETR_CHECK_ARG(det_bits && gt_bits && num_objects && inter, "bdetr_mask_inter: null pointer");
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MSK_MAX_N && M > 0 && M <= MSK_MAX_M && mask_layout_ok(Hm, Wm),
                    "bdetr_mask_inter: bad sizes B=%d N=%d M=%d Hm=%d Wm=%d (limits: B in [1, 65535], N in [1, %d], M in [1, %d], Hm in [1, %d], "
                    "Wm in [1, %d])", B, N, M, Hm, Wm, MSK_MAX_N, MSK_MAX_M, MI_MAX_DIM, MI_MAX_DIM / 64);
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
    BDETR_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MSK_MAX_N && M > 0 && M <= MSK_MAX_M && C >= 3 && C <= MSK_MAX_C && T > 0 &&
                    T <= MSK_MAX_T && A > 0 && A <= MSK_MAX_A && max_dets > 0,
                    "bdetr_mask_match_coco_inter: bad sizes B=%d N=%d M=%d C=%d T=%d A=%d max_dets=%d (limits: B <= 65535, N <= %d, M <= %d, "
                    "C in [3, %d], T in [1, %d], A in [1, %d], max_dets >= 1)", B, N, M, C, T, A, max_dets, MSK_MAX_N, MSK_MAX_M, MSK_MAX_C,
                    MSK_MAX_T, MSK_MAX_A);
    const size_t Np = (size_t)((N + 3) & ~3), Mp = (size_t)((M + 3) & ~3);
    const size_t base = Np * 24 + Mp * 8 + ((Np + Mp + 7) & ~(size_t)7);
    BDETR_CHECK_ARG(base <= MSK_LDS_LIMIT, "bdetr_mask_match_coco_inter: N=%d M=%d need %zu bytes of LDS per image; the limit is %zu", N, M, base,
                    MSK_LDS_LIMIT);
    const size_t staged = base + 4 * (size_t)N * M;
    mask_thresholds thr;
    for (int t = 0; t <= MSK_MAX_T; ++t) thr.v[t] = t < T ? thresholds[t] : 2.0;
    if (staged <= MSK_LDS_LIMIT)
        hipLaunchKernelGGL(mask_match_coco_inter_kernel<true>, dim3(B, A), dim3(64 * T), staged, (hipStream_t)stream, score, label, inter, det_pop,
                           gt_label, gt_pop, gt_crowd, gt_area, num_objects, image_hw, pix, area_ranges, thr, B, N, M, C, T, max_dets, order,
                           class_rank, tp_bits, ig_bits, matched_gt, gt_count);
    else
        hipLaunchKernelGGL(mask_match_coco_inter_kernel<false>, dim3(B, A), dim3(64 * T), base, (hipStream_t)stream, score, label, inter, det_pop,
                           gt_label, gt_pop, gt_crowd, gt_area, num_objects, image_hw, pix, area_ranges, thr, B, N, M, C, T, max_dets, order,
                           class_rank, tp_bits, ig_bits, matched_gt, gt_count);
    return bdetr_launch_status("mask_match_coco_inter");
}
