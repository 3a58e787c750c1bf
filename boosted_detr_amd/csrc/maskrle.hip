// maskrle.hip - COCO run-length encoding of bitmasks on gfx950 (K27, K28, include/bdetr.h): the number of runs of every mask of a
// batch, and the runs themselves.  Input is the layout of K19-K22 (maskimage.hip): uint64 [Hm, Wm] per mask, pixel (x, y) is bit
// x mod 64 of word [y, x div 64].  Only the pixels with y < h_b and x < w_b are looked at: nothing relies on the zero padding.
// kernels.mask_rle_encode chains K27, a prefix sum and K28; evaluation.CocoResults is the user.
//
// The rule is COCO's rleEncode: the pixels in column-major order p = x h + y, `counts` the lengths of the alternating runs starting
// with a run of zeros.  A TRANSITION is a p whose pixel differs from pixel p - 1 (pixel -1 counts as 0); a mask with T transitions
// has T + 1 counts.  Integers only: two calls give the same bits, and no atomics touch an output.
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int RLE_THREADS = 256;
constexpr int RLE_WAVES = RLE_THREADS / 64;
constexpr int RLE_MAX_DIM = 4096;         // image extents (K19's limit)
constexpr int RLE_MAX_COLS = RLE_MAX_DIM; // 64 Wm

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the bits of word column wd that are columns of a w pixel wide image
__device__ __forceinline__ u64 column_mask(int wd, int w) {
    const int left = w - wd * 64;
    return left >= 64 ? ~0ull : left <= 0 ? 0ull : (1ull << left) - 1ull;
}

struct image_extent {
    int h, w;
};
__device__ __forceinline__ image_extent load_extent(const int32_t* image_hw, int b, int Hm, int Wm) {
    return {min(max(image_hw[2 * b], 0), Hm), min(max(image_hw[2 * b + 1], 0), Wm * 64)};      // never past the buffers (as K19)
}

// ---------------------------------------------------------------------------------------------------------------------
// K27: bits [B,N,Hm,Wm] -> n_counts [B,N] = T + 1 (0 for a mask that is not kept)
// ---------------------------------------------------------------------------------------------------------------------
// Bit-parallel: the pixel before (x, y) in column-major order is (x, y - 1), so for y >= 1 the transitions of 64 columns of row y
// are row[y] ^ row[y - 1]; for y = 0 it is (x - 1, h - 1): row h - 1 moved up by one column, the carry crossing the word boundary
// and column 0 taking 0.  T is the sum of the popcounts, masked to x < w.
template <int VEC>
struct rle_words;
template <>
struct rle_words<1> {
    u64 x;
    __device__ __forceinline__ void load(const u64* p, int64_t c) { x = p[c]; }
    __device__ __forceinline__ int differ(const rle_words& o, int wd, int w) const { return __popcll((x ^ o.x) & column_mask(wd, w)); }
};
template <>
struct rle_words<2> {
    ulonglong2 v;
    __device__ __forceinline__ void load(const u64* p, int64_t c) { v = reinterpret_cast<const ulonglong2*>(p)[c]; }      // 16 bytes
    __device__ __forceinline__ int differ(const rle_words& o, int wd, int w) const {
        return __popcll((v.x ^ o.v.x) & column_mask(wd, w)) + __popcll((v.y ^ o.v.y) & column_mask(wd + 1, w));
    }
};

// One workgroup per mask.  The rows 1 .. h - 1 are one flat stream of words from HBM (VEC = 2: 16-byte loads, Wm even, so a load
// never straddles a row and the row above is the load Wm / 2 chunks earlier); the row above comes through the caches, it was
// streamed Wm words earlier by this same workgroup.  Row 0 is Wm words and is done by the first Wm lanes.
template <int VEC>
__global__ __launch_bounds__(RLE_THREADS) void mask_rle_count_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ image_hw,
                                                                     const uint8_t* __restrict__ keep, int N, int Hm, int Wm,
                                                                     int32_t* __restrict__ n_counts) {
    __shared__ int s_part[RLE_WAVES];
    const int o = blockIdx.x, tid = threadIdx.x;
    if (keep && !keep[o]) {                                      // uniform
        if (tid == 0) n_counts[o] = 0;
        return;
    }
    const image_extent e = load_extent(image_hw, o / N, Hm, Wm);
    const int h = e.h, w = e.w;
    const u64* p = bits + (int64_t)o * Hm * Wm;
    int acc = 0;
    if (h > 0 && tid < Wm) {                                     // row 0 against row h - 1 moved up by one column
        const u64* last = p + (int64_t)(h - 1) * Wm;
        const u64 pred = (last[tid] << 1) | (tid ? last[tid - 1] >> 63 : 0ull);
        acc = __popcll((p[tid] ^ pred) & column_mask(tid, w));
    }
    const int row = Wm / VEC;                                    // chunks per row
    const int step = RLE_THREADS % row;
    int cw = tid % row;                                          // this lane's chunk within its row
    for (int64_t c = row + tid, end = (int64_t)h * row; c < end; c += RLE_THREADS) {
        rle_words<VEC> cur, above;
        cur.load(p, c);
        above.load(p, c - row);
        acc += cur.differ(above, cw * VEC, w);
        cw += step;
        if (cw >= row) cw -= row;
    }
    acc = wave_sum_int(acc);
    if ((tid & 63) == 0) s_part[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        int T = 0;
#pragma unroll
        for (int k = 0; k < RLE_WAVES; ++k) T += s_part[k];
        n_counts[o] = T + 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K28: bits [B,N,Hm,Wm], offset [B N + 1] -> counts
// ---------------------------------------------------------------------------------------------------------------------
// 64 x 64 bit transpose over a wave: lane l gives row l (bit c = column c) and gets column l (bit r = row r).  Six butterfly
// steps: lanes s apart swap the off-diagonal s x s blocks.
__device__ __forceinline__ u64 transpose64(u64 v, int lane) {
    constexpr u64 LOW[6] = {0x00000000FFFFFFFFull, 0x0000FFFF0000FFFFull, 0x00FF00FF00FF00FFull,
                            0x0F0F0F0F0F0F0F0Full, 0x3333333333333333ull, 0x5555555555555555ull};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int s = 32 >> k;
        const u64 m = LOW[k];
        const u64 other = __shfl_xor(v, s, 64);
        v = (lane & s) ? (((other >> s) & m) | (v & ~m)) : ((v & m) | ((other & m) << s));
    }
    return v;
}

// A wave walks the 64 columns of word column wd down the image in blocks of 64 rows: lane l loads row 64 yb + l, the transpose
// hands lane l its column x = 64 wd + l (bit j = row 64 yb + j), and the column's transitions inside the block are
// col ^ (col << 1 | carry), carry being the pixel before the block's first in column-major order: the column's own row 64 yb - 1,
// or for yb = 0 pixel (x - 1, h - 1) (0 for x = 0).  sink(yb, t) gets the transition bits of the lane's column (0 for x >= w).
// Every lane of the wave must call it: the transpose shuffles.
template <class Sink>
__device__ __forceinline__ void walk_columns(const u64* __restrict__ p, int Wm, int h, int w, int wd, int lane, Sink&& sink) {
    const int x = wd * 64 + lane;
    const bool inside = x < w;
    u64 carry = 0ull;
    if (inside && x > 0 && h > 0) carry =(p[(int64_t)(h - 1) * Wm + ((x - 1) >> 6)] >> ((x - 1) & 63)) & 1ull;
    for (int yb = 0; yb * 64 < h; ++yb) {
        const int y = yb * 64 + lane, rows = min(64, h - yb * 64);
        const u64 col = transpose64(y < h ? p[(int64_t)y * Wm + wd] : 0ull, lane);
        u64 t = col ^ ((col << 1) | carry);
        if (rows < 64) t &= (1ull << rows) - 1ull;
        carry = col >> 63;
        sink(yb, inside ? t : 0ull);
    }
}

// One workgroup per mask, a wave per word column in turn.  First walk: the transitions per column into LDS; a workgroup scan makes
// them the columns' first slots (column-major order is ascending x, then ascending y).  Second walk: every transition's position p
// goes to its slot, and h w to slot T.  Last, in place from the top chunk down: counts[i] = pos[i] - pos[i - 1] (pos[-1] = 0); a chunk
// reads its own slots and the one below before any lower chunk is written.  The mask is read twice, the second time from the caches.
// Nothing is written outside counts[offset[o] : offset[o + 1]], whatever offset holds.
__global__ __launch_bounds__(RLE_THREADS) void mask_rle_encode_kernel(const u64* __restrict__ bits, const int32_t* __restrict__ image_hw,
                                                                      const uint8_t* __restrict__ keep, const int64_t* __restrict__ offset,
                                                                      int N, int Hm, int Wm, int64_t total, int32_t* counts) {
    __shared__ int s_slot[RLE_MAX_COLS];
    __shared__ int s_wave[RLE_WAVES];
    __shared__ int s_T;
    const int o = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (keep && !keep[o]) return;                                // uniform
    const int64_t off0 = offset[o], off1 = offset[o + 1];
    if (off0 < 0 || off1 <= off0 || off1 > total) return;        // uniform: no span, or one outside the buffer
    const int n = (int)min(off1 - off0, (int64_t)RLE_MAX_DIM * RLE_MAX_DIM + 1);
    int32_t* out = counts + off0;
    const image_extent e = load_extent(image_hw, o / N, Hm, Wm);
    const int h = e.h, w = e.w;
    const u64* p = bits + (int64_t)o * Hm * Wm;
    const int wpr = (w + 63) >> 6, cols = wpr * 64;              // <= RLE_MAX_COLS

    for (int wd = wave; wd < wpr; wd += RLE_WAVES) {
        int cnt = 0;
        walk_columns(p, Wm, h, w, wd, lane, [&](int, u64 t) { cnt += __popcll(t); });
        s_slot[wd * 64 + lane] = cnt;
    }
    __syncthreads();

    // exclusive scan of s_slot[0 : cols]: a lane sums `per` consecutive columns, the workgroup scans the 256 sums
    const int per = (cols + RLE_THREADS - 1) / RLE_THREADS, lo = min(tid * per, cols), hi = min(lo + per, cols);
    int mine = 0;
    for (int k = lo; k < hi; ++k) mine += s_slot[k];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    int before = incl - mine;
    for (int k = 0; k < wave; ++k) before += s_wave[k];
    if (tid == RLE_THREADS - 1) s_T = before + mine;
    for (int k = lo; k < hi; ++k) {
        const int c = s_slot[k];
        s_slot[k] = before;
        before += c;
    }
    __syncthreads();
    const int T = s_T;

    for (int wd = wave; wd < wpr; wd += RLE_WAVES) {
        const int x = wd * 64 + lane;
        int slot = s_slot[x];
        walk_columns(p, Wm, h, w, wd, lane, [&](int yb, u64 t) {
            const int base = x * h + yb * 64;                    // < 2^24
            while (t) {
                if (slot < n) out[slot] = base + __builtin_ctzll(t);
                ++slot;
                t &= t - 1ull;
            }
        });
    }
    if (tid == 0 && T < n) out[T] = h * w;
    __syncthreads();                                             // the positions are visible to the whole workgroup

    const int nn = min(T + 1, n);
    for (int cb = (nn - 1) / RLE_THREADS * RLE_THREADS; cb >= 0; cb -= RLE_THREADS) {
        const int i = cb + tid;
        int pos = 0, below = 0;
        if (i < nn) {
            pos = out[i];
            below = i ? out[i - 1] : 0;
        }
        __syncthreads();
        if (i < nn) out[i] = pos - below;
    }
}

bool rle_sizes_ok(int B, int N, int Hm, int Wm) {
    return B > 0 && N > 0 && (int64_t)B * N <= (1 << 24) && Hm >= 1 && Hm <= RLE_MAX_DIM && Wm >= 1 && Wm <= RLE_MAX_DIM / 64;
}

}  // namespace

extern "C" int bdetr_mask_rle_count(const uint64_t* bits, const int32_t* image_hw, const uint8_t* keep, int B, int N, int Hm, int Wm,
                                    int32_t* n_counts, void* stream) {
    BDETR_CHECK_ARG(bits && image_hw && n_counts, "bdetr_mask_rle_count: null pointer (only keep may be null)");
    BDETR_CHECK_ARG(rle_sizes_ok(B, N, Hm, Wm),
                    "bdetr_mask_rle_count: bad sizes B=%d N=%d Hm=%d Wm=%d (limits: B, N >= 1, B N <= 2^24, Hm in [1, %d], Wm in [1, %d])", B, N,
                    Hm, Wm, RLE_MAX_DIM, RLE_MAX_DIM / 64);
    const u64* p = reinterpret_cast<const u64*>(bits);
    // 16-byte loads need an even Wm (no load straddles a row, every mask starts on 16 bytes) and a 16-byte aligned base
    if (Wm % 2 == 0 && (uintptr_t)bits % 16 == 0)
        hipLaunchKernelGGL(mask_rle_count_kernel<2>, dim3((unsigned)(B * N)), dim3(RLE_THREADS), 0, (hipStream_t)stream, p, image_hw, keep, N, Hm,
                           Wm, n_counts);
    else
        hipLaunchKernelGGL(mask_rle_count_kernel<1>, dim3((unsigned)(B * N)), dim3(RLE_THREADS), 0, (hipStream_t)stream, p, image_hw, keep, N, Hm,
                           Wm, n_counts);
    return bdetr_launch_status("mask_rle_count");
}

extern "C" int bdetr_mask_rle_encode(const uint64_t* bits, const int32_t* image_hw, const uint8_t* keep, const int64_t* offset, int B, int N,
                                     int Hm, int Wm, int64_t total, int32_t* counts, void* stream) {
    BDETR_CHECK_ARG(bits && image_hw && offset && (counts || total == 0),
                    "bdetr_mask_rle_encode: null pointer (only keep may be null, and counts with total = 0)");
    BDETR_CHECK_ARG(rle_sizes_ok(B, N, Hm, Wm) && total >= 0,
                    "bdetr_mask_rle_encode: bad sizes B=%d N=%d Hm=%d Wm=%d total=%lld (limits: B, N >= 1, B N <= 2^24, Hm in [1, %d], "
                    "Wm in [1, %d], total >= 0)", B, N, Hm, Wm, (long long)total, RLE_MAX_DIM, RLE_MAX_DIM / 64);
    if (total == 0) return 0;                                    // no mask is kept: nothing to write
    hipLaunchKernelGGL(mask_rle_encode_kernel, dim3((unsigned)(B * N)), dim3(RLE_THREADS), 0, (hipStream_t)stream,
                       reinterpret_cast<const u64*>(bits), image_hw, keep, offset, N, Hm, Wm, (long long)total, counts);
    return bdetr_launch_status("mask_rle_encode");
}
