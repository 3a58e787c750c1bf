// panoptic.hip - the HBM-bound pieces of the panoptic head for gfx950: bilinear NHWC
// resize, channel LayerNormalization + leaky ReLU on channel counts that are not multiples of 4, column-block
// copies (channel concatenation / padding) and the final NHWC -> NCHW transpose.  The convolutions of the head
// (Conv2D k=2, Conv2DTranspose k=2 as a padded conv with flipped taps, Conv2D k=3 s=4) run on igemm.hip with the
// channel dimension zero-padded to a multiple of 4.
//
// Replaces: panoptic_neck.py:20-21 (Reshape + Resizing), 118-121 / 164-167 (LayerNormalization + ReLU(negative_slope)),
// 33-45 (Concatenate), 46-47 (transpose + reshape); transformers.py:519 (LayerNormalization of PanopticAttention).
//
// Training the head (DETR(train_panoptic_head=True)) adds the adjoints of these pieces - LayerNorm + leaky ReLU backward with
// fixed-order dgamma / dbeta partials, the bilinear resize backward as a gather, NCHW -> NHWC of the incoming mask gradient -, the
// device pack of the Keras-layout conv variables into padded OHWI kernels (and its adjoint for the weight gradients), and the mask
// loss (sigmoid focal + DICE over the matched queries, DETR's panoptic head; the reference defines none).  No float atomics.
#include "common.h"

namespace {

// tf.keras.layers.Resizing(bilinear): half-pixel centres, no antialias, edge clamp; C % 4 == 0 (padded)
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const float* __restrict__ in, int B, int h, int w, int C4,
                                                              float* __restrict__ out, int H, int W) {
    const int64_t n = (int64_t)B * H * W * C4;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4); int64_t t = i / C4;
        const int ox = (int)(t % W); t /= W; const int oy = (int)(t % H); const int b = (int)(t / H);
        const float fy = ((float)oy + 0.5f) * sy - 0.5f, fx = ((float)ox + 0.5f) * sx - 0.5f;
        const float fy0 = floorf(fy), fx0 = floorf(fx);
        const int y0 = max((int)fy0, 0), y1 = min((int)fy0 + 1, h - 1);
        const int x0 = max((int)fx0, 0), x1 = min((int)fx0 + 1, w - 1);
        const float ly = fy - fy0, lx = fx - fx0;
        const f32x4* base = reinterpret_cast<const f32x4*>(in) + (int64_t)b * h * w * C4;
        const f32x4 p00 = base[((int64_t)y0 * w + x0) * C4 + c4], p01 = base[((int64_t)y0 * w + x1) * C4 + c4];
        const f32x4 p10 = base[((int64_t)y1 * w + x0) * C4 + c4], p11 = base[((int64_t)y1 * w + x1) * C4 + c4];
        const f32x4 top = p00 + (p01 - p00) * lx, bot = p10 + (p11 - p10) * lx;
        reinterpret_cast<f32x4*>(out)[i] = top + (bot - top) * ly;
    }
}

// one wave per row: LayerNormalization over the first C of ld columns (biased variance), y = leaky(gamma * xhat + beta),
// columns C .. ldo-1 of the output row are written as zeros (channel padding for the next convolution)
__global__ __launch_bounds__(256) void layernorm_act_kernel(const float* __restrict__ x, int64_t rows, int C, int ldx,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float slope,
                                                            float* __restrict__ out, int ldo) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * ldx;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c = lane; c < C; c += 64) { const float t = xr[c] - mean; q += t * t; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    float* orow = out + row * ldo;
    for (int c = lane; c < ldo; c += 64) {
        float v = 0.f;
        if (c < C) { v = (xr[c] - mean) * rstd * gamma[c] + beta[c]; v = v >= 0.f ? v : v * slope; }
        orow[c] = v;
    }
}

// dst[r][col0 + c] = src[r][c] for c < C
__global__ __launch_bounds__(256) void copy_cols_kernel(const float* __restrict__ src, int64_t rows, int C, int lds_, float* __restrict__ dst, int ldd, int col0) {
    const int64_t n = rows * C;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % C); const int64_t r = i / C;
        dst[r * ldd + col0 + c] = src[r * lds_ + c];
    }
}

// out[b][c][p] = in[b][p][c] (c < C of ldin columns)
__global__ __launch_bounds__(256) void nhwc_to_nchw_kernel(const float* __restrict__ in, int B, int P, int C, int ldin, float* __restrict__ out) {
    const int64_t n = (int64_t)B * C * P;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int p = (int)(i % P); int64_t t = i / P; const int c = (int)(t % C); const int b = (int)(t / C);
        out[i] = in[((int64_t)b * P + p) * ldin + c];
    }
}

// ---- backward (train_panoptic_head) ----

constexpr int LNB_MAXJ = 8;             // columns per lane: C <= 512
constexpr int LNB_ROWS_PER_BLOCK = 16;  // 4 rows per wave: the 96 x 96 maps give ~600 workgroups
constexpr int LNB_MAX_BLOCKS = 1024;

static inline int lnb_chunks(int64_t rows) {
    int64_t n = cdiv64(rows, LNB_ROWS_PER_BLOCK);
    if (n > LNB_MAX_BLOCKS) n = LNB_MAX_BLOCKS;
    return (int)(n < 1 ? 1 : n);
}

// adjoint of layernorm_act_kernel: one wave per row (mean / rstd recomputed in the forward's order, slope chosen by the sign of
// gamma * xhat + beta exactly as the forward computed it); dx over ldx columns (0 beyond C); per-block partial dgamma / dbeta
// [nblk][C] (each wave keeps its rows' sums in registers, the block's four waves are folded in wave order - no atomics)
__global__ __launch_bounds__(256) void layernorm_act_bwd_kernel(const float* __restrict__ x, int64_t rows, int C, int ldx,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, float eps, float slope,
                                                                const float* __restrict__ dout, int ldo, float* __restrict__ dx,
                                                                float* __restrict__ part_g, float* __restrict__ part_b, int64_t rows_per_block) {
    __shared__ float red[2][4][LNB_MAXJ * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ag[LNB_MAXJ], ab[LNB_MAXJ];
#pragma unroll
    for (int j = 0; j < LNB_MAXJ; ++j) { ag[j] = 0.f; ab[j] = 0.f; }
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = min(rows, r0 + rows_per_block);
    for (int64_t row = r0 + wave; row < r1; row += 4) {
        const float* xr = x + row * ldx;
        float s = 0.f;
        for (int c = lane; c < C; c += 64) s += xr[c];
        const float mean = wave_sum(s) / (float)C;
        float q = 0.f;
        for (int c = lane; c < C; c += 64) { const float t = xr[c] - mean; q += t * t; }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
        const float* gr = dout + row * ldo;
        float xh[LNB_MAXJ], dh[LNB_MAXJ];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int j = 0; j < LNB_MAXJ; ++j) {
            const int c = lane + 64 * j;
            xh[j] = 0.f; dh[j] = 0.f;
            if (c < C) {
                const float v = (xr[c] - mean) * rstd * gamma[c] + beta[c];
                const float gp = v >= 0.f ? gr[c] : gr[c] * slope;
                xh[j] = (xr[c] - mean) * rstd;
                ag[j] += gp * xh[j]; ab[j] += gp;
                dh[j] = gp * gamma[c];
                s1 += dh[j]; s2 += dh[j] * xh[j];
            }
        }
        const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
        float* dr = dx + row * ldx;
#pragma unroll
        for (int j = 0; j < LNB_MAXJ; ++j) {
            const int c = lane + 64 * j;
            if (c < C) dr[c] = rstd * (dh[j] - m1 - xh[j] * m2);
        }
        for (int c = C + lane; c < ldx; c += 64) dr[c] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < LNB_MAXJ; ++j) { red[0][wave][j * 64 + lane] = ag[j]; red[1][wave][j * 64 + lane] = ab[j]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const float g = ((red[0][0][c] + red[0][1][c]) + red[0][2][c]) + red[0][3][c];
        const float b = ((red[1][0][c] + red[1][1][c]) + red[1][2][c]) + red[1][3][c];
        part_g[(int64_t)blockIdx.x * C + c] = g;
        part_b[(int64_t)blockIdx.x * C + c] = b;
    }
}

// dgamma[c] = sum_k part_g[k][c] (same for dbeta): one wave per column, lane l sums the blocks l, l + 64, ... in order, then the
// wave's fixed butterfly - the same order on every run
__global__ __launch_bounds__(64) void layernorm_act_bwd_fold_kernel(const float* __restrict__ part_g, const float* __restrict__ part_b, int nblk, int C,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x, lane = threadIdx.x;
    float g = 0.f, b = 0.f;
    for (int k = lane; k < nblk; k += 64) { g += part_g[(int64_t)k * C + c]; b += part_b[(int64_t)k * C + c]; }
    g = wave_sum(g);
    b = wave_sum(b);
    if (lane == 0) { dgamma[c] = g; dbeta[c] = b; }
}

// weight of input row `i` (of n) in output row `o` (of N) of resize_bilinear_kernel's interpolation (s = n / N)
__device__ __forceinline__ float resize_tap_weight(int o, int i, int n, float s) {
    const float f = ((float)o + 0.5f) * s - 0.5f;
    const float f0 = floorf(f);
    const int i0 = max((int)f0, 0), i1 = min((int)f0 + 1, n - 1);
    const float l = f - f0;
    return (i0 == i ? 1.f - l : 0.f) + (i1 == i ? l : 0.f);
}

// adjoint of resize_bilinear_kernel as a gather: din[b][iy][ix] = sum over the output pixels that read (iy, ix) of their weight * dout
__global__ __launch_bounds__(256) void resize_bilinear_bwd_kernel(const float* __restrict__ dout, int B, int H, int W, int C4,
                                                                  float* __restrict__ din, int h, int w) {
    const int64_t n = (int64_t)B * h * w * C4;
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c4 = (int)(i % C4); int64_t t = i / C4;
        const int ix = (int)(t % w); t /= w; const int iy = (int)(t % h); const int b = (int)(t / h);
        // output rows whose sample position f = (o + .5) * s - .5 lies in [iy - 1, iy + 1) (+1 of slack each side; the edges take the clamped rows)
        const int oy0 = iy == 0 ? 0 : max(0, (int)floorf(((float)iy - 0.5f) / sy - 0.5f) - 1);
        const int oy1 = iy == h - 1 ? H - 1 : min(H - 1, (int)ceilf(((float)iy + 1.5f) / sy - 0.5f) + 1);
        const int ox0 = ix == 0 ? 0 : max(0, (int)floorf(((float)ix - 0.5f) / sx - 0.5f) - 1);
        const int ox1 = ix == w - 1 ? W - 1 : min(W - 1, (int)ceilf(((float)ix + 1.5f) / sx - 0.5f) + 1);
        const f32x4* base = reinterpret_cast<const f32x4*>(dout) + (int64_t)b * H * W * C4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int oy = oy0; oy <= oy1; ++oy) {
            const float wy = resize_tap_weight(oy, iy, h, sy);
            if (wy == 0.f) continue;
            f32x4 row = {0.f, 0.f, 0.f, 0.f};
            for (int ox = ox0; ox <= ox1; ++ox) {
                const float wx = resize_tap_weight(ox, ix, w, sx);
                if (wx != 0.f) row += base[((int64_t)oy * W + ox) * C4 + c4] * wx;
            }
            acc += row * wy;
        }
        reinterpret_cast<f32x4*>(din)[i] = acc;
    }
}

// out[b][p][c] = in[b][c][p] for c < C, 0 for C <= c < ldo (adjoint of nhwc_to_nchw_kernel)
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float* __restrict__ in, int B, int P, int C, float* __restrict__ out, int ldo) {
    const int64_t n = (int64_t)B * P * ldo;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % ldo); const int64_t t = i / ldo; const int p = (int)(t % P); const int b = (int)(t / P);
        out[i] = c < C ? in[((int64_t)b * C + c) * P + p] : 0.f;
    }
}

// Keras-layout element of the kernel behind padded OHWI entry (o, r, s, i): HWIO [R][S][Cin][K], or (transpose) the
// Conv2DTranspose kernel [R][S][K][Cin] read with flipped taps
__device__ __forceinline__ int64_t keras_tap(int o, int r, int s, int i, int R, int S, int Cin, int K, int transpose) {
    return transpose ? (((int64_t)(R - 1 - r) * S + (S - 1 - s)) * K + o) * Cin + i : (((int64_t)r * S + s) * Cin + i) * K + o;
}

// w[Kp][R][S][Cp] (zeros beyond K / Cin), b[Kp] (zeros beyond K)
__global__ __launch_bounds__(256) void conv_weight_pack_kernel(const float* __restrict__ kernel, const float* __restrict__ bias, int R, int S, int Cin, int K,
                                                               int transpose, int Cp, int Kp, float* __restrict__ w, float* __restrict__ b) {
    const int64_t nw = (int64_t)Kp * R * S * Cp, n = nw + Kp;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        if (e >= nw) { const int o = (int)(e - nw); b[o] = o < K ? bias[o] : 0.f; continue; }
        const int i = (int)(e % Cp); int64_t t = e / Cp; const int s = (int)(t % S); t /= S; const int r = (int)(t % R); const int o = (int)(t / R);
        w[e] = (o < K && i < Cin) ? kernel[keras_tap(o, r, s, i, R, S, Cin, K, transpose)] : 0.f;
    }
}

// adjoint of the pack: the true-channel entries of the padded dw [Kp][R][S][Cp] / db [Kp] in the variables' Keras layout
__global__ __launch_bounds__(256) void conv_weight_unpack_kernel(const float* __restrict__ dw, const float* __restrict__ db, int R, int S, int Cin, int K,
                                                                 int transpose, int Cp, float* __restrict__ dkernel, float* __restrict__ dbias) {
    const int64_t nw = (int64_t)R * S * Cin * K, n = nw + K;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        if (e >= nw) { if (dbias) dbias[e - nw] = db[e - nw]; continue; }
        if (!dkernel) continue;
        int o, r, s, i;
        if (transpose) {          // [kh][kw][o][i]
            i = (int)(e % Cin); int64_t t = e / Cin; o = (int)(t % K); t /= K; const int kw = (int)(t % S), kh = (int)(t / S);
            r = R - 1 - kh; s = S - 1 - kw;
        } else {                  // [r][s][i][o]
            o = (int)(e % K); int64_t t = e / K; i = (int)(t % Cin); t /= Cin; s = (int)(t % S); r = (int)(t / S);
        }
        dkernel[e] = dw[(((int64_t)o * R + r) * S + s) * Cp + i];
    }
}

__device__ __forceinline__ float block_sum256(float v, float* lds) {
    // fixed order: wave sums, then waves 0..3
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

// one workgroup per (query n, image b): the object m < n_b matched to n (MatchingLoss.last_match), sigmoid focal loss (mean over the P
// pixels) + DICE of the logits row against masks[b][m]; the row's loss and its gradient (zero rows for unmatched queries)
__global__ __launch_bounds__(256) void mask_loss_rows_kernel(const float* __restrict__ logits, const float* __restrict__ masks, const int* __restrict__ match,
                                                             const int* __restrict__ num_objects, int M, int N, int P, float alpha, float gamma,
                                                             float mask_weight, float loss_scale, float* __restrict__ row_loss, float* __restrict__ dlogits) {
    __shared__ float lds[4];
    const int n = blockIdx.x, b = blockIdx.y;
    const int nb = min(max(num_objects[b], 0), M);
    int m = -1;
    for (int k = 0; k < nb; ++k) if (match[(int64_t)b * M + k] == n) { m = k; break; }
    const float* x = logits + ((int64_t)b * N + n) * P;
    float* dx = dlogits ? dlogits + ((int64_t)b * N + n) * P : nullptr;
    if (m < 0) {
        if (dx) for (int p = threadIdx.x; p < P; p += 256) dx[p] = 0.f;
        if (threadIdx.x == 0) row_loss[(int64_t)b * N + n] = 0.f;
        return;
    }
    const float* t = masks + ((int64_t)b * M + m) * P;
    float sf = 0.f, spt = 0.f, sp = 0.f, st = 0.f;
    for (int p = threadIdx.x; p < P; p += 256) {
        const float xv = x[p], tv = t[p];
        const float e = expf(-fabsf(xv));
        const float pr = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float qr = xv >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
        const float ce = fmaxf(xv, 0.f) - xv * tv + log1pf(e);
        const float omp = tv * qr + (1.f - tv) * pr;                       // 1 - p_t
        const float af = tv * alpha + (1.f - tv) * (1.f - alpha);
        sf += af * powf(omp, gamma) * ce;
        spt += pr * tv; sp += pr; st += tv;
    }
    sf = block_sum256(sf, lds); spt = block_sum256(spt, lds); sp = block_sum256(sp, lds); st = block_sum256(st, lds);
    const float num = 2.f * spt + 1.f, den = sp + st + 1.f;
    if (threadIdx.x == 0) row_loss[(int64_t)b * N + n] = sf / (float)P + (1.f - num / den);
    if (!dx) return;
    const float coef = loss_scale * mask_weight / (float)max(nb, 1);
    for (int p = threadIdx.x; p < P; p += 256) {
        const float xv = x[p], tv = t[p];
        const float e = expf(-fabsf(xv));
        const float pr = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        const float qr = xv >= 0.f ? e / (1.f + e) : 1.f / (1.f + e);
        const float pq = pr * qr;                                           // dsigma / dx
        const float ce = fmaxf(xv, 0.f) - xv * tv + log1pf(e);
        const float omp = tv * qr + (1.f - tv) * pr;
        const float af = tv * alpha + (1.f - tv) * (1.f - alpha);
        const float domp = -(2.f * tv - 1.f) * pq;                          // d(1 - p_t) / dx
        const float dfocal = af * (gamma * powf(omp, gamma - 1.f) * domp * ce + powf(omp, gamma) * (pr - tv));
        const float ddice = -(2.f * tv * den - num) / (den * den) * pq;
        dx[p] = coef * (dfocal / (float)P + ddice);
    }
}

// loss[b] = mask_weight * sum_n row_loss[b][n] / max(n_b, 1), n in order
__global__ __launch_bounds__(64) void mask_loss_fold_kernel(const float* __restrict__ row_loss, const int* __restrict__ num_objects, int B, int M, int N,
                                                            float mask_weight, float* __restrict__ loss) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float s = 0.f;
    for (int n = 0; n < N; ++n) s += row_loss[(int64_t)b * N + n];
    loss[b] = mask_weight * s / (float)max(min(max(num_objects[b], 0), M), 1);
}

}  // namespace

extern "C" int bdetr_resize_bilinear_nhwc(const float* in, int B, int h, int w, int C, float* out, int H, int W, void* stream) {
    BDETR_CHECK_ARG(in && out && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "bdetr_resize_bilinear_nhwc: bad arguments (C %% 4 == 0)");
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(ew_grid((int64_t)B * H * W * (C / 4), 256, 1)), dim3(256), 0, (hipStream_t)stream, in, B, h, w, C / 4, out, H, W);
    return bdetr_launch_status("resize_bilinear_nhwc");
}

extern "C" int bdetr_layernorm_act_fwd(const float* x, int64_t rows, int C, int ldx, const float* gamma, const float* beta, float eps, float slope,
                                       float* out, int ldo, void* stream) {
    BDETR_CHECK_ARG(x && gamma && beta && out && rows > 0 && C > 0 && ldx >= C && ldo >= C, "bdetr_layernorm_act_fwd: bad arguments");
    hipLaunchKernelGGL(layernorm_act_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, rows, C, ldx, gamma, beta, eps, slope, out, ldo);
    return bdetr_launch_status("layernorm_act_fwd");
}

extern "C" int bdetr_copy_cols(const float* src, int64_t rows, int C, int ld_src, float* dst, int ld_dst, int dst_col0, void* stream) {
    BDETR_CHECK_ARG(src && dst && rows > 0 && C > 0 && ld_src >= C && dst_col0 >= 0 && ld_dst >= dst_col0 + C, "bdetr_copy_cols: bad arguments");
    hipLaunchKernelGGL(copy_cols_kernel, dim3(ew_grid(rows * C, 256, 4)), dim3(256), 0, (hipStream_t)stream, src, rows, C, ld_src, dst, ld_dst, dst_col0);
    return bdetr_launch_status("copy_cols");
}

extern "C" int bdetr_nhwc_to_nchw(const float* in, int B, int P, int C, int ld_in, float* out, void* stream) {
    BDETR_CHECK_ARG(in && out && B > 0 && P > 0 && C > 0 && ld_in >= C, "bdetr_nhwc_to_nchw: bad arguments");
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(ew_grid((int64_t)B * P * C, 256, 4)), dim3(256), 0, (hipStream_t)stream, in, B, P, C, ld_in, out);
    return bdetr_launch_status("nhwc_to_nchw");
}

extern "C" int bdetr_layernorm_act_bwd_chunks(int64_t rows) { return rows > 0 ? lnb_chunks(rows) : -1; }

extern "C" int bdetr_layernorm_act_bwd(const float* x, int64_t rows, int C, int ldx, const float* gamma, const float* beta, float eps, float slope,
                                       const float* dout, int ldo, float* dx, float* part_g, float* part_b, float* dgamma, float* dbeta, void* stream) {
    BDETR_CHECK_ARG(x && gamma && beta && dout && dx && part_g && part_b && dgamma && dbeta && rows > 0 && C > 0 && C <= LNB_MAXJ * 64 && ldx >= C && ldo >= C,
                    "bdetr_layernorm_act_bwd: bad arguments (C <= %d)", LNB_MAXJ * 64);
    hipStream_t st = (hipStream_t)stream;
    const int nblk = lnb_chunks(rows);
    hipLaunchKernelGGL(layernorm_act_bwd_kernel, dim3((unsigned)nblk), dim3(256), 0, st, x, rows, C, ldx, gamma, beta, eps, slope, dout, ldo, dx,
                       part_g, part_b, cdiv64(rows, nblk));
    if (int e = bdetr_launch_status("layernorm_act_bwd")) return e;
    hipLaunchKernelGGL(layernorm_act_bwd_fold_kernel, dim3((unsigned)C), dim3(64), 0, st, part_g, part_b, nblk, C, dgamma, dbeta);
    return bdetr_launch_status("layernorm_act_bwd_fold");
}

extern "C" int bdetr_resize_bilinear_nhwc_bwd(const float* dout, int B, int H, int W, int C, float* din, int h, int w, void* stream) {
    BDETR_CHECK_ARG(dout && din && B > 0 && h > 0 && w > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0, "bdetr_resize_bilinear_nhwc_bwd: bad arguments (C %% 4 == 0)");
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(ew_grid((int64_t)B * h * w * (C / 4), 256, 1)), dim3(256), 0, (hipStream_t)stream, dout, B, H, W, C / 4, din, h, w);
    return bdetr_launch_status("resize_bilinear_nhwc_bwd");
}

extern "C" int bdetr_nchw_to_nhwc(const float* in, int B, int P, int C, float* out, int ld_out, void* stream) {
    BDETR_CHECK_ARG(in && out && B > 0 && P > 0 && C > 0 && ld_out >= C, "bdetr_nchw_to_nhwc: bad arguments");
    hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(ew_grid((int64_t)B * P * ld_out, 256, 4)), dim3(256), 0, (hipStream_t)stream, in, B, P, C, out, ld_out);
    return bdetr_launch_status("nchw_to_nhwc");
}

extern "C" int bdetr_conv_weight_pack(const float* kernel, const float* bias, int R, int S, int Cin, int K, int transpose, int Cp, int Kp,
                                      float* w, float* b, void* stream) {
    BDETR_CHECK_ARG(kernel && bias && w && b && R > 0 && S > 0 && Cin > 0 && K > 0 && Cp >= Cin && Kp >= K, "bdetr_conv_weight_pack: bad arguments");
    hipLaunchKernelGGL(conv_weight_pack_kernel, dim3(ew_grid((int64_t)Kp * R * S * Cp + Kp, 256, 4)), dim3(256), 0, (hipStream_t)stream,
                       kernel, bias, R, S, Cin, K, transpose, Cp, Kp, w, b);
    return bdetr_launch_status("conv_weight_pack");
}

extern "C" int bdetr_conv_weight_unpack(const float* dw, const float* db, int R, int S, int Cin, int K, int transpose, int Cp,
                                        float* dkernel, float* dbias, void* stream) {
    BDETR_CHECK_ARG(dw && db && R > 0 && S > 0 && Cin > 0 && K > 0 && Cp >= Cin, "bdetr_conv_weight_unpack: bad arguments");
    hipLaunchKernelGGL(conv_weight_unpack_kernel, dim3(ew_grid((int64_t)R * S * Cin * K + K, 256, 4)), dim3(256), 0, (hipStream_t)stream,
                       dw, db, R, S, Cin, K, transpose, Cp, dkernel, dbias);
    return bdetr_launch_status("conv_weight_unpack");
}

extern "C" int bdetr_mask_loss(const float* logits, const float* masks, const int* match, const int* num_objects, int B, int M, int N, int P,
                               float alpha, float gamma, float mask_weight, float loss_scale, float* row_loss, float* loss, float* dlogits, void* stream) {
    BDETR_CHECK_ARG(logits && masks && match && num_objects && row_loss && loss && B > 0 && M > 0 && N > 0 && P > 0 && N <= 65535 && B <= 65535,
                    "bdetr_mask_loss: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mask_loss_rows_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, st, logits, masks, match, num_objects, M, N, P, alpha, gamma,
                       mask_weight, loss_scale, row_loss, dlogits);
    if (int e = bdetr_launch_status("mask_loss_rows")) return e;
    hipLaunchKernelGGL(mask_loss_fold_kernel, dim3((unsigned)cdiv64(B, 64)), dim3(64), 0, st, row_loss, num_objects, B, M, N, mask_weight, loss);
    return bdetr_launch_status("mask_loss_fold");
}
