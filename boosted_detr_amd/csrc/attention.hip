// attention.hip - fused multi-head attention core for gfx950 (head dim 32; exact fp32 MFMA or three split 16-bit MFMA products).
//
// Replaces transformers.py:86-97 (MatMulQueryKey -> Rescaling(1/sqrt(d)) -> softmax -> mask of ones
// -> MatMulQueryValue) and its autodiff.  The [B,h,q,k] score tensor is never written to HBM:
// K/V (forward) or the streamed operand pair (backward) move through LDS in 64-row chunks and the
// softmax runs online in registers.
//
// Orientation trick (64-lane wavefronts, v_mfma_f32_32x32x2_f32): every product is arranged so that
// the softmax axis sits on the MFMA *row* index, which the 32x32 accumulator layout keeps inside a
// lane's 16 registers (+ the partner lane l^32).  Forward computes S^T = K Q^T (lane column = one
// query), so the row max / row sum are 15 in-register ops and one shuffle; the exponentiated tile is
// already the B operand of O^T += V^T P^T - P never touches LDS.  The backward uses the same layout
// twice: once with queries on the columns (dQ) and once with keys on the columns (dK, dV).
//
// Arithmetic (AR, chosen per launch from the library's GEMM policy, include/bdetr.h): 0 = exact fp32 (v_mfma_f32_32x32x2_f32,
// 64 cycles per 32x32x2: a 32-deep tile product costs 1,024 cycles); 2 = split-f16 forward / 1 = split-bf16 gradients - the
// streamed chunk is split into hi + lo 16-bit halves ONCE when it is written to LDS, the column operand once per kernel, an
// accumulator tile right before it is consumed, and a tile product is 2 x 3 v_mfma_f32_32x32x16 (192 cycles).  Same split
// arithmetic as the convolutions (csrc/p16.h: hi = half(x), lo = half(x - hi), one accumulator).  Measured round 3: the fp32
// kernels were MFMA-bound at ~50 % of the fp32 MFMA peak.
//
// Layouts: q/k/v/dq/dk/dv are [B, n, h*32] (head h at columns 32h..32h+31, exactly what the Dense
// projections produce); o/do are [B, h, q, 32] (the layout the reference reshapes without a
// permute, transformers.py:100); lse/dvec are [B, h, q].
#include "common.h"
#include "p16.h"
#include <stdlib.h>

namespace bdgemm { int gemm_mode(); }      // igemm.hip: the library's arithmetic policy (BDETR_GEMM_*)

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 abf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 af16x8 __attribute__((ext_vector_type(8)));
enum { AR_FP32 = 0, AR_BF16 = 1, AR_F16 = 2 };

constexpr int AD = 32;            // head dimension
constexpr int ALD = AD + 4;       // LDS row stride (floats): conflict-free 16-byte row reads
constexpr int CH = 64;            // streamed rows per chunk
constexpr int COLS_PER_BLOCK = 128;
// Chunks of look-ahead of the streamed operand pair (a ring of register sets).  Measured round 4 (-DBDETR_ATTN_PF=3 against 1, whole step,
// three alternating runs each on one box): 604.1 against 604.9 images/s - with three workgroups resident per CU the other workgroups
// cover a chunk's HBM round trip already; 1 keeps the registers.  Measured again after the softmax change (40 -> 20 VALU instructions per MFMA): depth 2
// equal (620 against 621 images/s), depth 3 slower (617; its backward launches 93 against 75 us: the extra register sets cost a resident workgroup).
#ifndef BDETR_ATTN_PF
#define BDETR_ATTN_PF 1
#endif
constexpr int APF = BDETR_ATTN_PF;

// exp() of the softmax as ONE v_exp_f32: the scores are kept in the log2 domain (scale * log2(e) folded into the one multiply they
// need anyway).  expf() is a ~12-instruction sequence and the forward kernel evaluated it 32 times per lane and chunk: 40 VALU
// instructions per MFMA, the kernel VALU-bound at 0.14 MFMA busy (PMC, round 4).  Relative error of 2^x' against e^x: the rounding of
// x' = x * log2(e), |x| * 6e-8 - the arguments are <= 0 and anything below -87 is zero either way.
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

__device__ __forceinline__ int crow(int e, int lh) { return (e & 3) + 8 * (e >> 2) + 4 * lh; }   // accumulator row of register e

// rows [r0, r0+64) of a strided matrix -> two float4 per thread (rows >= n are zero-filled) -> LDS [64][ALD].
// Split in two so that the next chunk's HBM loads are in flight while the current chunk is computed.
struct ChunkRegs { f32x4 v[2]; };
__device__ __forceinline__ ChunkRegs fetch_chunk(const float* __restrict__ base, int64_t stride, int r0, int n) {
    ChunkRegs c;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = threadIdx.x + 256 * p;
        const int row = v >> 3, c4 = v & 7;
        const int rr = min(r0 + row, n - 1);                               // clamped address, value masked below: no branch around the load
        f32x4 val = *reinterpret_cast<const f32x4*>(base + (int64_t)rr * stride + 4 * c4);
        if (r0 + row >= n) val = f32x4{0.f, 0.f, 0.f, 0.f};
        c.v[p] = val;
    }
    return c;
}
__device__ __forceinline__ void store_chunk(float* __restrict__ lds, const ChunkRegs& c) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = threadIdx.x + 256 * p;
        *reinterpret_cast<f32x4*>(lds + (v >> 3) * ALD + 4 * (v & 7)) = c.v[p];
    }
}

// 16 values X[col][16*lh + s] of this lane's column (or zeros when the column is out of range)
__device__ __forceinline__ void load_col_regs(float (&r)[16], const float* __restrict__ base, int64_t stride, int col, bool ok, int lh) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok) v = *reinterpret_cast<const f32x4*>(base + (int64_t)col * stride + 16 * lh + 4 * c);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[4 * c + e] = v[e];
    }
}

// tile[i][j] = sum_d R[32t+i][d] * C[j][d]  with C held per lane as creg[s] = C[j][16*lh+s]
__device__ __forceinline__ f32x16 row_times_col(const float* __restrict__ sR, int t, const float (&creg)[16], int li, int lh) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    f32x4 a[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = *reinterpret_cast<const f32x4*>(sR + (32 * t + li) * ALD + 16 * lh + 4 * c);
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s >> 2][s & 3], creg[s], acc, 0, 0, 0);
    return acc;
}

// acc[d][j] += sum_r R[32t+r][d] * T[r][j]   with T in accumulator layout (register e = row crow(e,lh))
__device__ __forceinline__ void accumulate_rt_tile(f32x16& acc, const float* __restrict__ sR, int t, const f32x16& tile, int li, int lh) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const float a = sR[(32 * t + crow(e, lh)) * ALD + li];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, tile[e], acc, 0, 0, 0);
    }
}

// ---------------- split (16-bit pair) flavour of the two tile products ----------------
// LDS image of a streamed 64 x 32 chunk: two planes (hi at +0, lo at +IMG_PLANE) of [64 rows][32 d] 16-bit = 64 bytes per row;
// the four 16-byte chunks of row r are XOR-ed with (r >> 2) & 3.  Row reads (ds_read_b128: lane = row) are then conflict-free -
// the 16 lanes of a read group see 4 distinct (r & 3) x 4 distinct chunks -, and so are the transposing reads
// (ds_read_b64_tr_b16: a half-wave reads 4 whole rows = 256 contiguous bytes, whatever the permutation inside a row).
constexpr int IMG_PLANE = CH * 64, IMG_BYTES = 2 * IMG_PLANE;
constexpr int SMEM_BYTES = IMG_BYTES > CH * ALD * 4 ? IMG_BYTES : CH * ALD * 4;

template <int AR>
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    if (AR == AR_F16) p16_split2_f16(x0, x1, hi, lo); else p16_split2_bf16(x0, x1, hi, lo);
}
template <int AR>
__device__ __forceinline__ f32x16 mfma3(const u32x4& ah, const u32x4& al, const u32x4& bh, const u32x4& bl, f32x16 acc) {
    if (AR == AR_F16) {
#define H8(v) __builtin_bit_cast(af16x8, v)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(H8(al), H8(bh), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(H8(ah), H8(bl), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(H8(ah), H8(bh), acc, 0, 0, 0);
#undef H8
    } else {
#define B8(v) __builtin_bit_cast(abf16x8, v)
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8(al), B8(bh), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8(ah), B8(bl), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(B8(ah), B8(bh), acc, 0, 0, 0);
#undef B8
    }
    return acc;
}
template <int AR>
__device__ __forceinline__ void store_chunk_split(unsigned char* __restrict__ img, const ChunkRegs& c) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int v = threadIdx.x + 256 * p, row = v >> 3, c4 = v & 7;
        unsigned h0, l0, h1, l1;
        split2<AR>(c.v[p][0], c.v[p][1], h0, l0);
        split2<AR>(c.v[p][2], c.v[p][3], h1, l1);
        const int off = row * 64 + (((c4 >> 1) ^ ((row >> 2) & 3)) << 4) + ((c4 & 1) << 3);
        *reinterpret_cast<u32x2*>(img + off) = u32x2{h0, h1};
        *reinterpret_cast<u32x2*>(img + IMG_PLANE + off) = u32x2{l0, l1};
    }
}
// a lane's 16 column values creg[s] = C[j][16 lh + s] -> the B fragments of the two 16-deep MFMA steps: step s2, element e <-> d = 16 lh + 8 s2 + e
struct ColFrag { u32x4 h[2], l[2]; };
template <int AR>
__device__ __forceinline__ ColFrag col_frag(const float (&r)[16]) {
    ColFrag f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
        for (int e = 0; e < 4; ++e) { unsigned h, l; split2<AR>(r[8 * s2 + 2 * e], r[8 * s2 + 2 * e + 1], h, l); f.h[s2][e] = h; f.l[s2][e] = l; }
    return f;
}
// tile[i][j] = sum_d R[32t+i][d] * C[j][d]: A fragment of step s2 = the 16 bytes of row 32t + li at d = 16 lh + 8 s2 (one ds_read_b128 per plane)
template <int AR>
__device__ __forceinline__ f32x16 row_times_col_split(const unsigned char* __restrict__ img, int t, const ColFrag& c, int li, int lh) {
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    const int row = 32 * t + li;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const int off = row * 64 + (((2 * lh + s2) ^ ((row >> 2) & 3)) << 4);
        const u32x4 ah = *reinterpret_cast<const u32x4*>(img + off), al = *reinterpret_cast<const u32x4*>(img + IMG_PLANE + off);
        acc = mfma3<AR>(ah, al, c.h[s2], c.l[s2], acc);
    }
    return acc;
}
// acc[d][j] += sum_r R[32t+r][d] * T[r][j], T in accumulator layout.  Step s2 takes T's registers 8 s2 .. 8 s2 + 7 as the B fragment:
// element e of lane half lh is row 16 s2 + 8 (e >> 2) + 4 lh + (e & 3), so the A fragment (lane = column d of R, transposed) must hold
// those same rows: two transposing reads per plane, each delivering 4 consecutive rows of the lane's column.
template <int AR>
__device__ __forceinline__ void accumulate_rt_tile_split(f32x16& acc, const unsigned char* __restrict__ img, int t, const f32x16& tile, int lane) {
    const int lh = lane >> 5, g16 = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        u32x4 bh, bl;
#pragma unroll
        for (int e = 0; e < 4; ++e) { unsigned h, l; split2<AR>(tile[8 * s2 + 2 * e], tile[8 * s2 + 2 * e + 1], h, l); bh[e] = h; bl[e] = l; }
        u32x2 ah2[2], al2[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int row = 32 * t + 16 * s2 + 8 * jj + 4 * lh + q;            // the block's row this lane addresses (columns 16 g16 + 4 p .. + 3)
            const int off = row * 64 + ((((2 * g16) + (p >> 1)) ^ ((row >> 2) & 3)) << 4) + ((p & 1) << 3);
            ah2[jj] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + off)));
            al2[jj] = __builtin_bit_cast(u32x2, __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(img + IMG_PLANE + off)));
        }
        const u32x4 ah = {ah2[0][0], ah2[0][1], ah2[1][0], ah2[1][1]}, al = {al2[0][0], al2[0][1], al2[1][0], al2[1][1]};
        acc = mfma3<AR>(ah, al, bh, bl, acc);
    }
}

// one interface over both flavours
template <int AR> struct ColOperand { float r[16]; ColFrag f; };
template <int AR>
__device__ __forceinline__ void chunk_store(unsigned char* smem, const ChunkRegs& c) {
    if constexpr (AR == AR_FP32) store_chunk(reinterpret_cast<float*>(smem), c); else store_chunk_split<AR>(smem, c);
}
template <int AR>
__device__ __forceinline__ f32x16 rows_x_col(const unsigned char* smem, int t, const ColOperand<AR>& c, int li, int lh) {
    if constexpr (AR == AR_FP32) return row_times_col(reinterpret_cast<const float*>(smem), t, c.r, li, lh);
    else return row_times_col_split<AR>(smem, t, c.f, li, lh);
}
template <int AR>
__device__ __forceinline__ void rowsT_x_tile(f32x16& acc, const unsigned char* smem, int t, const f32x16& tile, int lane) {
    if constexpr (AR == AR_FP32) accumulate_rt_tile(acc, reinterpret_cast<const float*>(smem), t, tile, lane & 31, lane >> 5);
    else accumulate_rt_tile_split<AR>(acc, smem, t, tile, lane);
}
template <int AR>
__device__ __forceinline__ void col_operand(ColOperand<AR>& c, const float* __restrict__ base, int64_t stride, int col, bool ok, int lh) {
    load_col_regs(c.r, base, stride, col, ok, lh);
    if constexpr (AR != AR_FP32) c.f = col_frag<AR>(c.r);
}

// ---------------- attention masks (include/bdetr.h K32 / K33) ----------------
// One compile-time parameter MK on the three tiled kernels (the way csrc/coco_match.h takes its F1 gate): MK_NONE compiles every
// line below away.  (KO beside it says whether the mask is key-only, sq == 0 - the common case, a padding mask: it then costs one
// register or 256 bytes of LDS, and must not pay the registers of the per-element loads of a full mask.)
// MK_F32 (multiply): the softmax runs over ALL keys, only the tile handed to the V^T P^T product (and, in the backward, to dV) is
// p * m, and dP is multiplied by m before dS.  MK_U8 (exclusion): a key whose byte is 0 has score -inf.
// The mask is [B or 1, h or 1, q or 1, nk] with element strides sb / sh / sq (0 on a broadcast axis) and unit stride along keys.
// Every element of a full mask is read by a one-element load of its own, predicated on key < nk and on the lane owning a row: mask
// rows are not 16-byte aligned in general (nk = 49) and nothing may read past a row's or the tensor's end.
enum { MK_NONE = 0, MK_F32 = 1, MK_U8 = 2 };
struct MaskArg { const void* p; int64_t sb, sh, sq; };
template <int MK> struct MaskElem { typedef float type; };
template <> struct MaskElem<MK_U8> { typedef unsigned char type; };
template <int MK>
__device__ __forceinline__ float mask_value(typename MaskElem<MK>::type x) {
    if constexpr (MK == MK_U8) return x != 0 ? 1.f : 0.f; else return x;
}
// Query on the lane (forward, dQ): mv[e] = mask[this lane's query][k0 + crow(e, lh)], 0 at keys >= nk and on lanes without a query.
// (base: the (image, head) plane, uniform; row0: this lane's row offset in it.  Offsets inside a plane are 32-bit - check_mask
// bounds the plane -, so an address is the scalar base plus ONE register.)
template <int MK>
__device__ __forceinline__ void mask_keys_of_query(float (&mv)[16], const typename MaskElem<MK>::type* __restrict__ base, unsigned row0, bool ok, int k0, int nk, int lh) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int kk = k0 + crow(e, lh);
        float x = 0.f;
        if (ok && kk < nk) x = mask_value<MK>(base[row0 + (unsigned)kk]);
        mv[e] = x;
    }
}
// A key-only mask (sq == 0: [B,1,1,k], [1,h,1,k]) is the same 64 values for every query of the workgroup: threads 0..63 stage the
// chunk's values in LDS beside the streamed chunk, and a lane reads its 16 as four broadcast 16-byte reads.
template <int MK>
__device__ __forceinline__ void mask_stage_keys(float* __restrict__ sM, const typename MaskElem<MK>::type* __restrict__ row, int c0, int nk) {
    if (threadIdx.x < CH) {
        const int kk = c0 + (int)threadIdx.x;
        sM[threadIdx.x] = kk < nk ? mask_value<MK>(row[kk]) : 0.f;
    }
}
__device__ __forceinline__ void mask_keys_staged(float (&mv)[16], const float* __restrict__ sM, int t, int lh) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(sM + 32 * t + 8 * c + 4 * lh);
#pragma unroll
        for (int e = 0; e < 4; ++e) mv[4 * c + e] = v[e];
    }
}

template <int AR, int MK, bool KO>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                       float* __restrict__ o, float* __restrict__ lse,
                                                       int h, int nq, int nk, float scale, MaskArg mk) {
    __shared__ __attribute__((aligned(16))) unsigned char sK[SMEM_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char sV[SMEM_BYTES];
    typedef typename MaskElem<MK>::type MT;
    float* sM = nullptr;
    if constexpr (MK != MK_NONE && KO) { __shared__ __attribute__((aligned(16))) float sMask[CH]; sM = sMask; }
    const int b = blockIdx.z, head = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int64_t D = (int64_t)h * AD;
    const int qi = blockIdx.x * COLS_PER_BLOCK + wave * 32 + li;
    const bool qok = qi < nq;
    ColOperand<AR> qr;
    col_operand<AR>(qr, q + (int64_t)b * nq * D + head * AD, D, qi, qok, lh);
    const float* kbase = k + (int64_t)b * nk * D + head * AD;
    const float* vbase = v + (int64_t)b * nk * D + head * AD;
    const MT* mbase = nullptr;                                  // this (image, head)'s mask plane; mrow: this lane's query row in it
    unsigned mrow = 0;
    if constexpr (MK != MK_NONE) {
        mbase = static_cast<const MT*>(mk.p) + (int64_t)b * mk.sb + (int64_t)head * mk.sh;
        mrow = qok ? (unsigned)qi * (unsigned)mk.sq : 0u;
    }
    auto mask_tile = [&](float (&mv)[16], int c0, int t) {
        if constexpr (KO) mask_keys_staged(mv, sM, t, lh); else mask_keys_of_query<MK>(mv, mbase, mrow, qok, c0 + 32 * t, nk, lh);
    };

    f32x16 oacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[e] = 0.f;
    float m = -INFINITY, l = 0.f;

    const float scale2 = scale * LOG2E;
    const bool wave_active = blockIdx.x * COLS_PER_BLOCK + wave * 32 < nq;      // wave-uniform: idle waves only help loading
    // the streamed chunks are fetched APF chunks ahead (see APF)
    ChunkRegs ck[APF], cv[APF];
#pragma unroll
    for (int p = 0; p < APF; ++p) {
        ck[p] = ChunkRegs{}; cv[p] = ChunkRegs{};
        if (p * CH < nk) { ck[p] = fetch_chunk(kbase, D, p * CH, nk); cv[p] = fetch_chunk(vbase, D, p * CH, nk); }
    }
    for (int c0 = 0; c0 < nk; c0 += CH) {
        __syncthreads();
        chunk_store<AR>(sK, ck[0]);
        chunk_store<AR>(sV, cv[0]);
        if constexpr (MK != MK_NONE && KO) mask_stage_keys<MK>(sM, mbase, c0, nk);
        __syncthreads();
#pragma unroll
        for (int p = 0; p + 1 < APF; ++p) { ck[p] = ck[p + 1]; cv[p] = cv[p + 1]; }
        if (c0 + APF * CH < nk) { ck[APF - 1] = fetch_chunk(kbase, D, c0 + APF * CH, nk); cv[APF - 1] = fetch_chunk(vbase, D, c0 + APF * CH, nk); }
        if (!wave_active) continue;
        f32x16 s[2];
        float cmax = -INFINITY;
        const bool full = c0 + CH <= nk;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            s[t] = rows_x_col<AR>(sK, t, qr, li, lh);              // S^T tile: rows = keys, column = this lane's query
#pragma unroll
            for (int e = 0; e < 16; ++e) s[t][e] *= scale2;        // log2 domain
        }
        if (!full) {                                               // (uniform branch: only the last chunk has ragged rows)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) if (!(c0 + 32 * t + crow(e, lh) < nk)) s[t][e] = -INFINITY;
        }
        if constexpr (MK == MK_U8) {                               // exclusion: the key takes no part in the softmax
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float mv[16];
                mask_tile(mv, c0, t);
#pragma unroll
                for (int e = 0; e < 16; ++e) s[t][e] = mv[e] != 0.f ? s[t][e] : -INFINITY;
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) cmax = fmaxf(cmax, s[t][e]);
        cmax = fmaxf(cmax, __shfl_xor(cmax, 32, 64));
        const float mn = fmaxf(m, cmax);
        // exclusion: while no key has been kept yet the running maximum is still -inf, and (-inf) - (-inf) is NaN: subtract 0 then
        // (alpha = 2^-inf = 0, every p = 2^-inf = 0).  With a finite maximum this is the unmasked arithmetic, bit for bit.
        float mref = mn;
        if constexpr (MK == MK_U8) mref = mn == -INFINITY ? 0.f : mn;
        const float alpha = exp2_fast(m - mref);
        float psum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) { const float p = exp2_fast(s[t][e] - mref); s[t][e] = p; psum += p; }
        psum += __shfl_xor(psum, 32, 64);
        l = l * alpha + psum;
        m = mn;
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[e] *= alpha;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if constexpr (MK == MK_F32) {                          // multiply: l above summed the unmasked p; only this tile is p * m
                float mv[16];
                mask_tile(mv, c0, t);
#pragma unroll
                for (int e = 0; e < 16; ++e) s[t][e] *= mv[e];
            }
            rowsT_x_tile<AR>(oacc, sV, t, s[t], lane);             // O^T += V^T P^T
        }
    }
    if (qok) {
        float inv = 1.0f / l;
        if constexpr (MK == MK_U8) if (!(l > 0.f)) { inv = 0.f; m = -INFINITY; }          // a row with no kept key: O = 0, lse = -inf
        float* orow = o + (((int64_t)b * h + head) * nq + qi) * AD;
#pragma unroll
        for (int e = 0; e < 16; ++e) orow[crow(e, lh)] = oacc[e] * inv;
        float lrow = m * LN2 + logf(l);                                                   // (m is a log2-domain maximum)
        if constexpr (MK == MK_U8) if (!(l > 0.f)) lrow = -INFINITY;
        if (lh == 0) lse[((int64_t)b * h + head) * nq + qi] = lrow;
    }
}

// dvec[row] = sum_d do[row][d] * o[row][d]   (rows = B*h*q, 32 columns): 8 lanes per row
__global__ __launch_bounds__(256) void attn_dvec_kernel(const float* __restrict__ o, const float* __restrict__ d_o, float* __restrict__ dvec, int64_t rows) {
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
    const int c4 = threadIdx.x & 7;
    float s = 0.f;
    if (row < rows) {
        const f32x4 a = reinterpret_cast<const f32x4*>(o)[row * 8 + c4], g = reinterpret_cast<const f32x4*>(d_o)[row * 8 + c4];
        s = a[0] * g[0] + a[1] * g[1] + a[2] * g[2] + a[3] * g[3];
    }
    s += __shfl_xor(s, 1, 64); s += __shfl_xor(s, 2, 64); s += __shfl_xor(s, 4, 64);
    if (row < rows && c4 == 0) dvec[row] = s;
}

// KCOL == false: columns = queries, streamed rows = keys     -> out1 = dQ
// KCOL == true : columns = keys,    streamed rows = queries  -> out1 = dK, out2 = dV
// With a mask (MK, above): dP = M * (dO V^T) and dV = (P * M)^T dO under the multiply rule - dS = P (dP - D) scale holds unchanged
// because sum_k P_k M_k (dO . V_k) = dO . O, so attn_dvec_kernel is the unmasked one -; under exclusion P is 0 at an excluded key, and
// a row with no kept key (lse = -inf) has P = 0 everywhere.  KCOL == false reads the mask as the forward does; KCOL == true owns one
// key per lane and streams queries, so it reads mask[q = c0 + r][k = ci]: consecutive lanes, consecutive addresses (a key-only mask:
// one value per lane, loaded once).
template <bool KCOL, int AR, int MK, bool KO>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                       const float* __restrict__ d_o, const float* __restrict__ lse, const float* __restrict__ dvec,
                                                       float* __restrict__ out1, float* __restrict__ out2,
                                                       int h, int nq, int nk, float scale, MaskArg mk) {
    __shared__ __attribute__((aligned(16))) unsigned char sR1[SMEM_BYTES];
    __shared__ __attribute__((aligned(16))) unsigned char sR2[SMEM_BYTES];
    __shared__ float sL[CH], sD[CH];
    typedef typename MaskElem<MK>::type MT;
    float* sM = nullptr;
    if constexpr (MK != MK_NONE && KO && !KCOL) { __shared__ __attribute__((aligned(16))) float sMask[CH]; sM = sMask; }
    const int b = blockIdx.z, head = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, lh = lane >> 5;
    const int64_t D = (int64_t)h * AD;
    const int ncol = KCOL ? nk : nq, nrow = KCOL ? nq : nk;
    const int ci = blockIdx.x * COLS_PER_BLOCK + wave * 32 + li;
    const bool cok = ci < ncol;
    const int64_t bh = (int64_t)b * h + head;

    // column-side operands in registers
    const float* c1base = (KCOL ? k : q) + (int64_t)b * ncol * D + head * AD;
    const float* c2base = KCOL ? (v + (int64_t)b * nk * D + head * AD) : (d_o + bh * nq * AD);
    const int64_t c2stride = KCOL ? D : AD;
    ColOperand<AR> c1r, c2r;
    col_operand<AR>(c1r, c1base, D, ci, cok, lh);
    col_operand<AR>(c2r, c2base, c2stride, ci, cok, lh);
    // streamed row-side operands
    const float* r1base = (KCOL ? q : k) + (int64_t)b * nrow * D + head * AD;
    const float* r2base = KCOL ? (d_o + bh * nq * AD) : (v + (int64_t)b * nk * D + head * AD);
    const int64_t r2stride = KCOL ? AD : D;

    float Lcol = 0.f, Dcol = 0.f;
    if (!KCOL && cok) { Lcol = lse[bh * nq + ci] * LOG2E; Dcol = dvec[bh * nq + ci]; }      // (log2 domain: see exp2_fast)
    const float scale2 = scale * LOG2E;
    const MT* mbase = nullptr;                                  // this (image, head)'s mask plane; mrow: this lane's query row in it (dQ kernel)
    unsigned mrow = 0;
    float mcol = 0.f;                                           // key-only mask of this lane's key (dK/dV kernel)
    if constexpr (MK != MK_NONE) {
        mbase = static_cast<const MT*>(mk.p) + (int64_t)b * mk.sb + (int64_t)head * mk.sh;
        if (!KCOL) mrow = cok ? (unsigned)ci * (unsigned)mk.sq : 0u;
        if (KCOL && KO && cok) mcol = mask_value<MK>(mbase[ci]);
    }
    // dK/dV under a key-only float mask: m is a constant of the lane's key j, so M * (dO V^T) = dO (m_j V_j)^T and dV_j = m_j sum_r p dO_r:
    // the V column is scaled once here, dV once at the end, and the loop below is the unmasked loop (m_j = 1: exact both times).
    constexpr bool COLSCALE = KCOL && KO && MK == MK_F32;
    if constexpr (COLSCALE) {
#pragma unroll
        for (int s = 0; s < 16; ++s) c2r.r[s] *= mcol;
        if constexpr (AR != AR_FP32) c2r.f = col_frag<AR>(c2r.r);
    }
    auto mask_tile = [&](float (&mv)[16], int c0, int t) {
        if constexpr (!KCOL) {
            if constexpr (KO) mask_keys_staged(mv, sM, t, lh); else mask_keys_of_query<MK>(mv, mbase, mrow, cok, c0 + 32 * t, nk, lh);
        } else if constexpr (!KO) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int qr = c0 + 32 * t + crow(e, lh);
                float x = 0.f;
                if (cok && qr < nq) x = mask_value<MK>(mbase[(unsigned)qr * (unsigned)mk.sq + (unsigned)ci]);
                mv[e] = x;
            }
        }
    };

    f32x16 acc1, acc2;
#pragma unroll
    for (int e = 0; e < 16; ++e) { acc1[e] = 0.f; acc2[e] = 0.f; }

    const bool wave_active = blockIdx.x * COLS_PER_BLOCK + wave * 32 < ncol;
    ChunkRegs c1[APF], c2[APF];                      // (fetched APF chunks ahead: see attn_fwd_kernel)
#pragma unroll
    for (int p = 0; p < APF; ++p) {
        c1[p] = ChunkRegs{}; c2[p] = ChunkRegs{};
        if (p * CH < nrow) { c1[p] = fetch_chunk(r1base, D, p * CH, nrow); c2[p] = fetch_chunk(r2base, r2stride, p * CH, nrow); }
    }
    for (int c0 = 0; c0 < nrow; c0 += CH) {
        __syncthreads();
        chunk_store<AR>(sR1, c1[0]);
        chunk_store<AR>(sR2, c2[0]);
        if (KCOL && threadIdx.x < CH) {
            const int qi = c0 + threadIdx.x;
            sL[threadIdx.x] = qi < nq ? lse[bh * nq + qi] * LOG2E : 0.f;
            sD[threadIdx.x] = qi < nq ? dvec[bh * nq + qi] : 0.f;
        }
        if constexpr (MK != MK_NONE && KO && !KCOL) mask_stage_keys<MK>(sM, mbase, c0, nk);
        __syncthreads();
#pragma unroll
        for (int p = 0; p + 1 < APF; ++p) { c1[p] = c1[p + 1]; c2[p] = c2[p + 1]; }
        if (c0 + APF * CH < nrow) { c1[APF - 1] = fetch_chunk(r1base, D, c0 + APF * CH, nrow); c2[APF - 1] = fetch_chunk(r2base, r2stride, c0 + APF * CH, nrow); }
        if (!wave_active) continue;
        const bool full = c0 + CH <= nrow;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x16 S = rows_x_col<AR>(sR1, t, c1r, li, lh);     // scores      (rows = streamed side)
            f32x16 G = rows_x_col<AR>(sR2, t, c2r, li, lh);     // dP          (same orientation)
            float mv[16];
            if constexpr (MK != MK_NONE && !(KCOL && KO)) mask_tile(mv, c0, t);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = 32 * t + crow(e, lh);
                const float me = (MK == MK_NONE || COLSCALE) ? 1.f : (KCOL && KO) ? mcol : mv[e];
                const float Lq = KCOL ? sL[r] : Lcol, Dq = KCOL ? sD[r] : Dcol;
                // (a select, not a branch on the uniform `full`: the branched form measured 98 against 77 us on the encoder shape)
                float p = (full || c0 + r < nrow) ? exp2_fast(S[e] * scale2 - Lq) : 0.f;
                if constexpr (MK == MK_U8) p = me != 0.f ? p : 0.f;        // (a select: 2^(s + inf) of a row with no kept key never multiplies)
                float g = G[e];
                if constexpr (MK == MK_F32 && !COLSCALE) g *= me;             // dP = M * (dO V^T)
                S[e] = p * (g - Dq) * scale;                     // dS (gradient w.r.t. the unscaled product)
                G[e] = p;
                if constexpr (MK == MK_F32 && !COLSCALE) G[e] = p * me;       // dV takes P * M
            }
            rowsT_x_tile<AR>(acc1, sR1, t, S, lane);             // dQ^T += K^T dS^T   |  dK^T += Q^T dS
            if (KCOL) rowsT_x_tile<AR>(acc2, sR2, t, G, lane);   // dV^T += dO^T P
        }
    }
    if (cok) {
        float* o1 = out1 + ((int64_t)b * ncol + ci) * D + head * AD;
#pragma unroll
        for (int e = 0; e < 16; ++e) o1[crow(e, lh)] = acc1[e];
        if (KCOL) {
            float* o2 = out2 + ((int64_t)b * ncol + ci) * D + head * AD;
#pragma unroll
            for (int e = 0; e < 16; ++e) o2[crow(e, lh)] = COLSCALE ? acc2[e] * mcol : acc2[e];
        }
    }
}

// BDETR_ATTN_SPLIT=0 keeps every attention product on the exact-fp32 MFMA (A/B measurements; recorded by bench.py when set)
bool attn_split_enabled() {
    static int on = -1;
    if (on < 0) { const char* e = getenv("BDETR_ATTN_SPLIT"); on = e ? atoi(e) != 0 : 1; }
    return on != 0;
}

int check_attn(const void* a, const void* b, const void* c, int B, int h, int nq, int nk, const char* who) {
    BDETR_CHECK_ARG(a && b && c, "%s: null pointer", who);
    BDETR_CHECK_ARG(B > 0 && h > 0 && nq > 0 && nk > 0 && B <= 65535 && h <= 65535, "%s: bad sizes B=%d h=%d nq=%d nk=%d", who, B, h, nq, nk);
    BDETR_CHECK_ARG(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 15) == 0 && ((uintptr_t)c & 15) == 0, "%s: operands must be 16-byte aligned", who);
    return 0;
}

// mask, its three element strides and the rule: checked before any launch.  The furthest element a kernel may address is
// (B-1) sb + (h-1) sh + (nq-1) sq + nk - 1; that sum has to exist as an int64.
int check_mask(const void* mask, int64_t sb, int64_t sh, int64_t sq, int mode, int B, int h, int nq, int nk, const char* who) {
    BDETR_CHECK_ARG(mask != nullptr, "%s: null mask", who);
    BDETR_CHECK_ARG(mode == BDETR_ATTN_MASK_MULTIPLY || mode == BDETR_ATTN_MASK_EXCLUDE, "%s: unknown mask mode %d", who, mode);
    BDETR_CHECK_ARG(sb >= 0 && sh >= 0 && sq >= 0, "%s: negative mask stride (%lld, %lld, %lld)", who, (long long)sb, (long long)sh, (long long)sq);
    int64_t a = 0, c = 0, d = 0, sum = 0;
    const bool overflow = __builtin_mul_overflow((int64_t)(B - 1), sb, &a) || __builtin_mul_overflow((int64_t)(h - 1), sh, &c) ||
                          __builtin_mul_overflow((int64_t)(nq - 1), sq, &d) || __builtin_add_overflow(a, c, &sum) ||
                          __builtin_add_overflow(sum, d, &sum) || __builtin_add_overflow(sum, (int64_t)nk, &sum) ||
                          sum > INT64_MAX / 4;                                       // (byte offsets of a float mask)
    BDETR_CHECK_ARG(!overflow, "%s: mask size x stride overflows (strides %lld, %lld, %lld)", who, (long long)sb, (long long)sh, (long long)sq);
    BDETR_CHECK_ARG(d + (int64_t)nk <= (int64_t)0x7fffffff, "%s: one (image, head) plane of the mask, (nq-1) sq + nk = %lld elements, exceeds 2^31 - 1",
                    who, (long long)(d + nk));
    BDETR_CHECK_ARG(mode != BDETR_ATTN_MASK_MULTIPLY || ((uintptr_t)mask & 3) == 0, "%s: a float mask must be 4-byte aligned", who);
    return 0;
}

// forward products follow the policy's forward arithmetic: split-f16 under BDETR_GEMM_SPLIT (operands are LayerNorm-scale
// projections and probabilities), split-bf16 under BDETR_GEMM_BF16X3, exact fp32 otherwise
template <int MK, bool KO>
void launch_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int h, int nq, int nk, float scale, MaskArg mk, hipStream_t st) {
    dim3 grid((nq + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK, h, B);
    const int mode = attn_split_enabled() ? bdgemm::gemm_mode() : BDETR_GEMM_FP32;
    if (mode == BDETR_GEMM_SPLIT) hipLaunchKernelGGL((attn_fwd_kernel<AR_F16, MK, KO>), grid, dim3(256), 0, st, q, k, v, o, lse, h, nq, nk, scale, mk);
    else if (mode == BDETR_GEMM_BF16X3) hipLaunchKernelGGL((attn_fwd_kernel<AR_BF16, MK, KO>), grid, dim3(256), 0, st, q, k, v, o, lse, h, nq, nk, scale, mk);
    else hipLaunchKernelGGL((attn_fwd_kernel<AR_FP32, MK, KO>), grid, dim3(256), 0, st, q, k, v, o, lse, h, nq, nk, scale, mk);
}

template <int MK, bool KO>
void launch_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o, const float* lse, float* dq, float* dk, float* dv,
                float* dvec_ws, int B, int h, int nq, int nk, float scale, MaskArg mk, hipStream_t st) {
    const int64_t rows = (int64_t)B * h * nq;
    hipLaunchKernelGGL(attn_dvec_kernel, dim3((unsigned)((rows * 8 + 255) / 256)), dim3(256), 0, st, o, d_o, dvec_ws, rows);
    // gradient products: split-bf16 (fp32 range) under every policy but BDETR_GEMM_FP32, like the conv / GEMM family
    const dim3 gq((nq + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK, h, B), gk((nk + COLS_PER_BLOCK - 1) / COLS_PER_BLOCK, h, B);
    if (!attn_split_enabled() || bdgemm::gemm_mode() == BDETR_GEMM_FP32 || bdgemm::gemm_mode() == BDETR_GEMM_BF16X6) {      // (bf16x6: the fp32-grade policy)
        hipLaunchKernelGGL((attn_bwd_kernel<false, AR_FP32, MK, KO>), gq, dim3(256), 0, st, q, k, v, d_o, lse, dvec_ws, dq, (float*)nullptr, h, nq, nk, scale, mk);
        hipLaunchKernelGGL((attn_bwd_kernel<true, AR_FP32, MK, KO>), gk, dim3(256), 0, st, q, k, v, d_o, lse, dvec_ws, dk, dv, h, nq, nk, scale, mk);
    } else {
        hipLaunchKernelGGL((attn_bwd_kernel<false, AR_BF16, MK, KO>), gq, dim3(256), 0, st, q, k, v, d_o, lse, dvec_ws, dq, (float*)nullptr, h, nq, nk, scale, mk);
        hipLaunchKernelGGL((attn_bwd_kernel<true, AR_BF16, MK, KO>), gk, dim3(256), 0, st, q, k, v, d_o, lse, dvec_ws, dk, dv, h, nq, nk, scale, mk);
    }
}

// x[b][hd][q][k] (contiguous [B,h,nq,nk]) against a mask with the fused kernels' broadcast strides, for the unfused attention path:
// fill == 0: out = x * m (float mask) or (m ? x : 0) (byte mask);  fill != 0 (byte mask only): out = m ? x : BDETR_ATTN_MASK_FILL.
template <int MK>
__global__ __launch_bounds__(256) void attn_mask_apply_kernel(const float* __restrict__ x, float* __restrict__ out, MaskArg mk, int h, int nq, int nk,
                                                              int64_t total, int fill) {
    typedef typename MaskElem<MK>::type MT;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int kk = (int)(i % nk);
    const int64_t r = i / nk;
    const int qi = (int)(r % nq);
    const int64_t bh = r / nq;
    const int hd = (int)(bh % h);
    const int64_t b = bh / h;
    const float m = mask_value<MK>(static_cast<const MT*>(mk.p)[b * mk.sb + hd * mk.sh + qi * mk.sq + kk]);
    const float xv = x[i];
    if constexpr (MK == MK_U8) out[i] = m != 0.f ? xv : (fill ? BDETR_ATTN_MASK_FILL : 0.f);
    else out[i] = xv * m;
}

}  // namespace

extern "C" int bdetr_attention_head_dim(void) { return AD; }

extern "C" int bdetr_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse,
                                   int B, int h, int nq, int nk, float scale, void* stream) {
    if (int e = check_attn(q, k, v, B, h, nq, nk, "bdetr_attention_fwd")) return e;
    BDETR_CHECK_ARG(o && lse, "bdetr_attention_fwd: null output");
    launch_fwd<MK_NONE, false>(q, k, v, o, lse, B, h, nq, nk, scale, MaskArg{nullptr, 0, 0, 0}, (hipStream_t)stream);
    return bdetr_launch_status("attention_fwd");
}

extern "C" int bdetr_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                   const float* lse, float* dq, float* dk, float* dv, float* dvec_ws,
                                   int B, int h, int nq, int nk, float scale, void* stream) {
    if (int e = check_attn(q, k, v, B, h, nq, nk, "bdetr_attention_bwd")) return e;
    BDETR_CHECK_ARG(o && d_o && lse && dq && dk && dv && dvec_ws, "bdetr_attention_bwd: null pointer");
    launch_bwd<MK_NONE, false>(q, k, v, o, d_o, lse, dq, dk, dv, dvec_ws, B, h, nq, nk, scale, MaskArg{nullptr, 0, 0, 0}, (hipStream_t)stream);
    return bdetr_launch_status("attention_bwd");
}

extern "C" int bdetr_attention_masked_fwd(const float* q, const float* k, const float* v, float* o, float* lse,
                                          int B, int h, int nq, int nk, float scale,
                                          const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, void* stream) {
    if (int e = check_attn(q, k, v, B, h, nq, nk, "bdetr_attention_masked_fwd")) return e;
    BDETR_CHECK_ARG(o && lse, "bdetr_attention_masked_fwd: null output");
    if (int e = check_mask(mask, mask_sb, mask_sh, mask_sq, mask_mode, B, h, nq, nk, "bdetr_attention_masked_fwd")) return e;
    const MaskArg mk{mask, mask_sb, mask_sh, mask_sq};
    hipStream_t st = (hipStream_t)stream;
    const bool ko = mask_sq == 0;                                      // key-only: its own instantiations (see MK)
    if (mask_mode == BDETR_ATTN_MASK_MULTIPLY) {
        if (ko) launch_fwd<MK_F32, true>(q, k, v, o, lse, B, h, nq, nk, scale, mk, st); else launch_fwd<MK_F32, false>(q, k, v, o, lse, B, h, nq, nk, scale, mk, st);
    } else {
        if (ko) launch_fwd<MK_U8, true>(q, k, v, o, lse, B, h, nq, nk, scale, mk, st); else launch_fwd<MK_U8, false>(q, k, v, o, lse, B, h, nq, nk, scale, mk, st);
    }
    return bdetr_launch_status("attention_masked_fwd");
}

extern "C" int bdetr_attention_masked_bwd(const float* q, const float* k, const float* v, const float* o, const float* d_o,
                                          const float* lse, float* dq, float* dk, float* dv, float* dvec_ws,
                                          int B, int h, int nq, int nk, float scale,
                                          const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, void* stream) {
    if (int e = check_attn(q, k, v, B, h, nq, nk, "bdetr_attention_masked_bwd")) return e;
    BDETR_CHECK_ARG(o && d_o && lse && dq && dk && dv && dvec_ws, "bdetr_attention_masked_bwd: null pointer");
    if (int e = check_mask(mask, mask_sb, mask_sh, mask_sq, mask_mode, B, h, nq, nk, "bdetr_attention_masked_bwd")) return e;
    const MaskArg mk{mask, mask_sb, mask_sh, mask_sq};
    hipStream_t st = (hipStream_t)stream;
    const bool ko = mask_sq == 0;
    if (mask_mode == BDETR_ATTN_MASK_MULTIPLY) {
        if (ko) launch_bwd<MK_F32, true>(q, k, v, o, d_o, lse, dq, dk, dv, dvec_ws, B, h, nq, nk, scale, mk, st);
        else launch_bwd<MK_F32, false>(q, k, v, o, d_o, lse, dq, dk, dv, dvec_ws, B, h, nq, nk, scale, mk, st);
    } else {
        if (ko) launch_bwd<MK_U8, true>(q, k, v, o, d_o, lse, dq, dk, dv, dvec_ws, B, h, nq, nk, scale, mk, st);
        else launch_bwd<MK_U8, false>(q, k, v, o, d_o, lse, dq, dk, dv, dvec_ws, B, h, nq, nk, scale, mk, st);
    }
    return bdetr_launch_status("attention_masked_bwd");
}

extern "C" int bdetr_attention_mask_apply(const float* x, float* out, int B, int h, int nq, int nk,
                                          const void* mask, int64_t mask_sb, int64_t mask_sh, int64_t mask_sq, int mask_mode, int fill, void* stream) {
    BDETR_CHECK_ARG(x && out, "bdetr_attention_mask_apply: null pointer");
    BDETR_CHECK_ARG(B > 0 && h > 0 && nq > 0 && nk > 0, "bdetr_attention_mask_apply: bad sizes B=%d h=%d nq=%d nk=%d", B, h, nq, nk);
    if (int e = check_mask(mask, mask_sb, mask_sh, mask_sq, mask_mode, B, h, nq, nk, "bdetr_attention_mask_apply")) return e;
    BDETR_CHECK_ARG(!fill || mask_mode == BDETR_ATTN_MASK_EXCLUDE, "bdetr_attention_mask_apply: fill needs the exclusion rule");
    const int64_t total = (int64_t)B * h * nq * nk;
    BDETR_CHECK_ARG((total + 255) / 256 <= 0x7fffffff, "bdetr_attention_mask_apply: %lld elements are too many", (long long)total);
    const MaskArg mk{mask, mask_sb, mask_sh, mask_sq};
    const dim3 grid((unsigned)((total + 255) / 256));
    if (mask_mode == BDETR_ATTN_MASK_MULTIPLY) hipLaunchKernelGGL((attn_mask_apply_kernel<MK_F32>), grid, dim3(256), 0, (hipStream_t)stream, x, out, mk, h, nq, nk, total, fill);
    else hipLaunchKernelGGL((attn_mask_apply_kernel<MK_U8>), grid, dim3(256), 0, (hipStream_t)stream, x, out, mk, h, nq, nk, total, fill);
    return bdetr_launch_status("attention_mask_apply");
}

