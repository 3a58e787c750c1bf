// groupnorm_rows.hip - BatchNormalization over ROW GROUPS for gfx950: x is [G * R][C] and group g (rows [g R, (g + 1) R)) is normalised
// with its own batch statistics, as G separate keras BatchNormalization calls on [R][C] would (prediction_heads.py:42,108,177 called
// once per decoder layer: model.py:179-186 with use_intermediate_losses).  The prediction heads of all decoder layers then run as ONE
// stacked tensor: one statistics launch, one apply launch and two backward launches per head, whatever G is.
//
// All fp32 in HBM, 16 bytes per lane, no atomics and no hand-off between workgroups: a workgroup owns (16 columns, one group) and
// reduces that group's R rows alone - 64 row phases in registers, then a fixed-order fp64 fold of the 64 phase partials in LDS - so
// no partial sum ever straddles a group boundary and every result is bit-reproducible.  What needs ALL groups of a column (the G
// chained moving-statistics updates; dgamma / dbeta) is done by the launch BEHIND the reduction, which finds the per-group results
// complete in HBM: the apply launch folds the moving statistics in group order, the backward apply launch sums the per-group
// gradient sums in group order.  Sized for the heads: R = batch x queries (a few thousand rows), C = 256 .. 1024.
#include "common.h"

namespace {

constexpr int SLAB = 16;        // columns per workgroup: 4 lanes x float4
constexpr int PHASES = 64;      // row phases per workgroup (256 threads)

// the BN affine map and input gradient with their fused multiply-adds spelled out, as in norm.hip
__device__ __forceinline__ float bn_affine(float v, float m, float rs, float g, float b) { return __builtin_fmaf(v - m, rs * g, b); }
__device__ __forceinline__ float bn_bwd_dx(float g, float xv, float m, float rs, float gm, float dg, float db, float inv_rows) {
    const float xh = (xv - m) * rs;
    const float t = __builtin_fmaf(-db, inv_rows, g);
    return __builtin_fmaf(-xh, dg * inv_rows, t) * (rs * gm);
}

struct RowStatFn {      // a = x, b = x * x
    const float* x;
    __device__ __forceinline__ void operator()(int64_t off, int, int, f32x4& a, f32x4& b) const {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + off);
        a = v; b = v * v;
    }
};

struct RowBwdFn {       // a = g, b = g * xhat (the group's own mean / rstd; stat_stride 0: constants shared by every group)
    const float* dout; const float* x; const float* mean; const float* rstd; int stat_stride;
    __device__ __forceinline__ void operator()(int64_t off, int g, int c, f32x4& a, f32x4& b) const {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(dout + off), xv = *reinterpret_cast<const f32x4*>(x + off);
        const f32x4 m = *reinterpret_cast<const f32x4*>(mean + (int64_t)g * stat_stride + c);
        const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + (int64_t)g * stat_stride + c);
        a = gv; b = gv * ((xv - m) * rs);
    }
};

// Column sums of two quantities over the R rows of group blockIdx.y, for the 16 columns of slab blockIdx.x.  The totals (fp64) of
// column `col` come back in threads 0..15 (col = slab * 16 + threadIdx.x, valid when col < C); other threads get zeros.
template <class F>
__device__ __forceinline__ void group_colsum2(const F& f, int64_t R, int C, double& ta, double& tb) {
    __shared__ float sa[PHASES * SLAB], sb[PHASES * SLAB];
    const int tid = threadIdx.x, cx = tid & 3, ry = tid >> 2;
    const int g = blockIdx.y, c = blockIdx.x * SLAB + cx * 4;
    f32x4 a = {0, 0, 0, 0}, b = {0, 0, 0, 0};
    if (c < C) {
        const int64_t base = (int64_t)g * R * C + c;
        int64_t r = ry;
        for (; r + 3 * PHASES < R; r += 4 * PHASES) {          // four rows' loads in flight per thread, fixed summation order
            f32x4 qa[4], qb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) f(base + (r + u * PHASES) * C, g, c, qa[u], qb[u]);
#pragma unroll
            for (int u = 0; u < 4; ++u) { a += qa[u]; b += qb[u]; }
        }
        for (; r < R; r += PHASES) { f32x4 qa, qb; f(base + r * C, g, c, qa, qb); a += qa; b += qb; }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) { sa[ry * SLAB + cx * 4 + e] = a[e]; sb[ry * SLAB + cx * 4 + e] = b[e]; }
    __syncthreads();
    ta = 0; tb = 0;
    if (tid < SLAB) {
        for (int p = 0; p < PHASES; ++p) { ta += (double)sa[p * SLAB + tid]; tb += (double)sb[p * SLAB + tid]; }
    }
}

__global__ __launch_bounds__(256) void bn_rows_stats_kernel(const float* __restrict__ x, int64_t R, int C, float eps,
                                                            float* __restrict__ mean, float* __restrict__ rstd, float* __restrict__ var_out,
                                                            int* guard) {
    double s, q;
    group_colsum2(RowStatFn{x}, R, C, s, q);
    const int col = blockIdx.x * SLAB + threadIdx.x;
    if (threadIdx.x < SLAB && col < C) {
        const double m = s / (double)R;
        double var = q / (double)R - m * m;          // biased, like bdetr_bn_stats(bessel = 0)
        if (var < 0) var = 0;
        const int64_t o = (int64_t)blockIdx.y * C + col;
        mean[o] = (float)m;
        rstd[o] = (float)(1.0 / sqrt(var + (double)eps));
        var_out[o] = (float)var;
        if (guard != nullptr && (!(fabs(m) <= 3.0e38) || !(var <= 3.0e38))) *guard = 1;      // (catches NaN too; see bn_finalize_kernel)
    }
}

// out = gamma * (x - mean_g) * rstd_g + beta, g = row / R.  With moving_mean != null the launch also leaves the moving statistics as G
// sequential keras calls would: mm <- momentum * mm + (1 - momentum) * mean_g for g = 0 .. G-1 (and the variance), unless the step's
// range guard is up - the statistics launch in front of this one raised it for non-finite statistics.
__global__ __launch_bounds__(256) void bn_rows_apply_kernel(const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ out,
                                                            int G, unsigned R, int C, int stat_stride, int64_t n4,
                                                            const float* __restrict__ var, float momentum, float* mmean, float* mvar, const int* guard) {
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    if (mmean != nullptr && (guard == nullptr || *guard == 0)) {
        for (int64_t c = gtid; c < C; c += gstride) {
            float mm = mmean[c], mv = mvar[c];
            for (int g = 0; g < G; ++g) {
                mm = mm * momentum + mean[(int64_t)g * C + c] * (1.f - momentum);
                mv = mv * momentum + var[(int64_t)g * C + c] * (1.f - momentum);
            }
            mmean[c] = mm; mvar[c] = mv;
        }
    }
    const unsigned c4n = (unsigned)C / 4;
    for (int64_t i = gtid; i < n4; i += gstride) {
        const unsigned row = (unsigned)(i / c4n), c = (unsigned)(i - (int64_t)row * c4n) * 4, g = row / R;
        const int64_t so = (int64_t)g * stat_stride + c;
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
        const f32x4 m = *reinterpret_cast<const f32x4*>(mean + so), rs = *reinterpret_cast<const f32x4*>(rstd + so);
        const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c), bt = *reinterpret_cast<const f32x4*>(beta + c);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = bn_affine(v[e], m[e], rs[e], gm[e], bt[e]);
        reinterpret_cast<f32x4*>(out)[i] = o;
    }
}

__global__ __launch_bounds__(256) void bn_rows_bwd_reduce_kernel(RowBwdFn f, int64_t R, int C, float* __restrict__ sum_g, float* __restrict__ sum_gx) {
    double a, b;
    group_colsum2(f, R, C, a, b);
    const int col = blockIdx.x * SLAB + threadIdx.x;
    if (threadIdx.x < SLAB && col < C) {
        sum_g[(int64_t)blockIdx.y * C + col] = (float)a;
        sum_gx[(int64_t)blockIdx.y * C + col] = (float)b;
    }
}

// dx from the row's OWN group's sums; dgamma / dbeta = the per-group sums added in group order (fp64)
__global__ __launch_bounds__(256) void bn_rows_bwd_apply_kernel(const float* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ mean,
                                                                const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ sum_g, const float* __restrict__ sum_gx, int frozen,
                                                                float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                                int G, unsigned R, int C, int stat_stride, int64_t n4, float inv_rows) {
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t c = gtid; c < C; c += gstride) {
        double a = 0, b = 0;
        for (int g = 0; g < G; ++g) { a += (double)sum_g[(int64_t)g * C + c]; b += (double)sum_gx[(int64_t)g * C + c]; }
        dbeta[c] = (float)a; dgamma[c] = (float)b;
    }
    const unsigned c4n = (unsigned)C / 4;
    for (int64_t i = gtid; i < n4; i += gstride) {
        const unsigned row = (unsigned)(i / c4n), c = (unsigned)(i - (int64_t)row * c4n) * 4, g = row / R;
        const int64_t so = (int64_t)g * stat_stride + c;
        const f32x4 gv = reinterpret_cast<const f32x4*>(dout)[i];
        const f32x4 rs = *reinterpret_cast<const f32x4*>(rstd + so), gm = *reinterpret_cast<const f32x4*>(gamma + c);
        f32x4 r;
        if (frozen) {
            r = gv * (rs * gm);
        } else {
            const f32x4 xv = reinterpret_cast<const f32x4*>(x)[i], m = *reinterpret_cast<const f32x4*>(mean + so);
            const f32x4 db = *reinterpret_cast<const f32x4*>(sum_g + (int64_t)g * C + c), dg = *reinterpret_cast<const f32x4*>(sum_gx + (int64_t)g * C + c);
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = bn_bwd_dx(gv[e], xv[e], m[e], rs[e], gm[e], dg[e], db[e], inv_rows);
        }
        reinterpret_cast<f32x4*>(dx)[i] = r;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool shape_ok(int G, int64_t R, int C) { return G > 0 && G <= 65535 && R > 0 && C > 0 && C % 4 == 0 && (int64_t)G * R < ((int64_t)1 << 31); }

}  // namespace

// ------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------
extern "C" int bdetr_bn_rows_stats(const float* x, int G, int64_t R, int C, float eps, float* mean, float* rstd, float* var, int* guard_flag,
                                   void* stream) {
    BDETR_CHECK_ARG(x && mean && rstd && var && shape_ok(G, R, C) && aligned16(x),
                    "bdetr_bn_rows_stats: bad arguments (C %% 4 == 0, G <= 65535, G * R < 2^31, 16-byte aligned x required)");
    hipLaunchKernelGGL(bn_rows_stats_kernel, dim3((C + SLAB - 1) / SLAB, G), dim3(256), 0, (hipStream_t)stream, x, R, C, eps, mean, rstd, var, guard_flag);
    return bdetr_launch_status("bn_rows_stats");
}

extern "C" int bdetr_bn_rows_apply(const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* out,
                                   int G, int64_t R, int C, int grouped_stats, const float* var, float momentum, float* moving_mean,
                                   float* moving_var, const int* guard_flag, void* stream) {
    BDETR_CHECK_ARG(x && mean && rstd && gamma && beta && out && shape_ok(G, R, C) && aligned16(x) && aligned16(out) && aligned16(mean) &&
                    aligned16(rstd) && aligned16(gamma) && aligned16(beta),
                    "bdetr_bn_rows_apply: bad arguments (C %% 4 == 0, G <= 65535, G * R < 2^31, 16-byte aligned tensors required)");
    BDETR_CHECK_ARG(moving_mean == nullptr || (moving_var && var && grouped_stats),
                    "bdetr_bn_rows_apply: the moving-statistics update needs moving_var and the per-group mean / var of bdetr_bn_rows_stats");
    const int64_t n4 = (int64_t)G * R * C / 4;
    hipLaunchKernelGGL(bn_rows_apply_kernel, dim3(ew_grid(n4, 256, 2)), dim3(256), 0, (hipStream_t)stream, x, mean, rstd, gamma, beta, out, G, (unsigned)R, C,
                       grouped_stats ? C : 0, n4, var, momentum, moving_mean, moving_var, guard_flag);
    return bdetr_launch_status("bn_rows_apply");
}

extern "C" int bdetr_bn_rows_bwd(const float* dout, const float* x, const float* mean, const float* rstd, const float* gamma, int grouped_stats,
                                 int frozen, float* dx, float* dgamma, float* dbeta, float* ws, int G, int64_t R, int C, void* stream) {
    BDETR_CHECK_ARG(dout && x && mean && rstd && gamma && dx && dgamma && dbeta && ws && shape_ok(G, R, C) && aligned16(dout) && aligned16(x) &&
                    aligned16(dx) && aligned16(mean) && aligned16(rstd) && aligned16(gamma) && aligned16(ws),
                    "bdetr_bn_rows_bwd: bad arguments (C %% 4 == 0, G <= 65535, G * R < 2^31, 16-byte aligned tensors required)");
    hipStream_t st = (hipStream_t)stream;
    const int stat_stride = grouped_stats ? C : 0;
    float* sum_g = ws; float* sum_gx = ws + (int64_t)G * C;          // ws: 2 * G * C floats
    hipLaunchKernelGGL(bn_rows_bwd_reduce_kernel, dim3((C + SLAB - 1) / SLAB, G), dim3(256), 0, st, RowBwdFn{dout, x, mean, rstd, stat_stride}, R, C,
                       sum_g, sum_gx);
    const int64_t n4 = (int64_t)G * R * C / 4;
    hipLaunchKernelGGL(bn_rows_bwd_apply_kernel, dim3(ew_grid(n4, 256, 2)), dim3(256), 0, st, dout, x, mean, rstd, gamma, sum_g, sum_gx, frozen, dx, dgamma,
                       dbeta, G, (unsigned)R, C, stat_stride, n4, 1.0f / (float)R);
    return bdetr_launch_status("bn_rows_bwd");
}
