// optim.hip - fused multi-tensor optimizer step for gfx950 (HBM-bound).
//
// Replaces the Keras optimizer the notebooks compile the model with
// (DETR_COCO.ipynb cell 26: SGD(momentum=.9, nesterov=True, clipnorm=.1)), SURVEY S15:
//   g  <- g * grad_scale ; g <- g * min(1, clipnorm/||g||_2)        (per tensor)
//   v  <- m*v - lr*g ;  w <- w + m*v - lr*g
// and the AdamW line next to it in the same cell (tfa.optimizers.AdamW = Keras Adam + decoupled weight decay), see adamw_apply_kernel.
#include "common.h"
#include "stream.h"

namespace {

struct TensorTriple { float* w; float* g; float* v; };

// one workgroup per (tensor, slab): deterministic per-slab partial sums of g^2
constexpr int SLAB = 16384;

// NT: the gradient loads carry the non-temporal hint (stream.h)
template <bool NT>
__global__ __launch_bounds__(256) void sqnorm_kernel(const uint64_t* __restrict__ ptrs, const int64_t* __restrict__ sizes,
                                                     const int64_t* __restrict__ slab_tensor, const int64_t* __restrict__ slab_first,
                                                     float* __restrict__ partial, int stride) {
    __shared__ float sh[4];
    const int64_t t = slab_tensor[blockIdx.x];
    const int64_t off = (blockIdx.x - slab_first[t]) * (int64_t)SLAB;
    const float* g = reinterpret_cast<const float*>(ptrs[(int64_t)stride * t + 1]);      // table rows: {w, g, ...} - 3 pointers for SGD, 4 for AdamW
    const int64_t n = sizes[t];
    float s = 0.f;
    // 16-byte loads over the slab's whole quads (every tensor's slot in the flat buffers is 16-byte aligned and a slab starts at a
    // multiple of 16,384 elements), the last 1-3 elements one by one: the 4-byte form ran at 2.1 TB/s (round 5)
    const int64_t end = min(n, off + SLAB), nq = (reinterpret_cast<uintptr_t>(g) & 15) == 0 ? (end - off) >> 2 : 0;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + off);
    for (int64_t q = threadIdx.x; q < nq; q += 256) { const f32x4 x = ld_stream<NT>(g4 + q); s += x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]; }
    for (int64_t i = off + 4 * nq + threadIdx.x; i < end; i += 256) { float x = ld_stream<NT>(g + i); s += x * x; }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

// guard (optional): raised when a tensor's gradient norm is not finite - a NaN / Inf born in the backward pass, which the loss
// check of the range guard cannot see; sgd_apply_kernel (the next launch) then applies nothing at all.
__global__ __launch_bounds__(256) void norm_final_kernel(const float* __restrict__ partial, const int64_t* __restrict__ slab_first, int ntensors,
                                                         float* __restrict__ norms, int* __restrict__ guard) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntensors) return;
    double s = 0;
    for (int64_t k = slab_first[t]; k < slab_first[t + 1]; ++k) s += partial[k];
    const float nrm = (float)sqrt(s);
    norms[t] = nrm;
    if (guard != nullptr && !(fabsf(nrm) <= 3.0e38f)) *guard = 1;
}

// NT: gradient and momentum loads non-temporal (their last use this step); NTS: the momentum store too (its next reader is a step away).
// The weight's load and store keep the default policy: the weight pack reads the weights next.
template <bool NT, bool NTS>
__global__ __launch_bounds__(256) void sgd_apply_kernel(const uint64_t* __restrict__ ptrs, const int64_t* __restrict__ sizes,
                                                        const int64_t* __restrict__ slab_tensor, const int64_t* __restrict__ slab_first,
                                                        const float* __restrict__ norms, const float* __restrict__ lr_p,
                                                        float momentum, float clipnorm, float grad_scale, const int* __restrict__ skip_flag) {
    if (skip_flag != nullptr && *skip_flag != 0) return;      // the step overflowed the f16 pair range / went non-finite: apply nothing
    const int64_t t = slab_tensor[blockIdx.x];
    const int64_t off = (blockIdx.x - slab_first[t]) * (int64_t)SLAB;
    float* w = reinterpret_cast<float*>(ptrs[3 * t + 0]);
    const float* g = reinterpret_cast<const float*>(ptrs[3 * t + 1]);
    float* v = reinterpret_cast<float*>(ptrs[3 * t + 2]);
    const int64_t n = sizes[t];
    const float lr = *lr_p;
    float scale = grad_scale;
    if (clipnorm > 0.f) {
        const float nrm = norms[t] * fabsf(grad_scale);
        if (nrm > clipnorm) scale *= clipnorm / nrm;
    }
    const bool aligned = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    const int64_t end = min(n, off + SLAB), nq = aligned ? (end - off) >> 2 : 0;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + off);
    f32x4* v4 = reinterpret_cast<f32x4*>(v + off);
    f32x4* w4 = reinterpret_cast<f32x4*>(w + off);
    for (int64_t q = threadIdx.x; q < nq; q += 256) {             // (the same arithmetic per element as the scalar tail below)
        const f32x4 gq = ld_stream<NT>(g4 + q), vq = ld_stream<NT>(v4 + q), wq = w4[q];
        f32x4 vn, wn;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float gi = gq[e] * scale;
            vn[e] = momentum * vq[e] - lr * gi;
            wn[e] = wq[e] + momentum * vn[e] - lr * gi;
        }
        st_stream<NTS>(v4 + q, vn); w4[q] = wn;
    }
    for (int64_t i = off + 4 * nq + threadIdx.x; i < end; i += 256) {
        const float gi = ld_stream<NT>(g + i) * scale;
        const float vn = momentum * ld_stream<NT>(v + i) - lr * gi;
        st_stream<NTS>(v + i, vn);
        w[i] = w[i] + momentum * vn - lr * gi;
    }
}

// One element of the AdamW step, in the op order include/bdetr.h documents; every product and sum is rounded on its own (no fma
// contraction: the same bits whichever path - quad or tail - an element takes, and an fp32 NumPy restatement can follow it exactly).
// IEEE sqrt and division: the update is HBM-bound, arithmetic is free.
struct AdamConsts { float lr_t, wd_t, b1, b2, omb1, omb2, eps, scale; bool decay; };

__device__ __forceinline__ void adamw_elem(const AdamConsts& c, float g, float& w, float& m, float& v) {
#pragma clang fp contract(off)
    const float gi = g * c.scale;
    float wi = w;
    if (c.decay) wi = wi - c.wd_t * wi;                      // decoupled: not multiplied by the learning rate
    const float mn = c.b1 * m + c.omb1 * gi;
    const float vn = c.b2 * v + c.omb2 * (gi * gi);
    m = mn; v = vn;
    w = wi - (c.lr_t * mn) / (sqrtf(vn) + c.eps);            // Keras' "epsilon hat": lr_t carries the bias correction
}

// Same shape as sgd_apply_kernel: one workgroup per (tensor, slab), 16-byte accesses over whole quads when all four pointers are
// 16-byte aligned, element-wise tail.  step_scalars = {lr_t, wd_t} in HBM (a captured segment replays with this step's values).
__global__ __launch_bounds__(256) void adamw_apply_kernel(const uint64_t* __restrict__ ptrs, const int64_t* __restrict__ sizes,
                                                          const int64_t* __restrict__ slab_tensor, const int64_t* __restrict__ slab_first,
                                                          const float* __restrict__ norms, const float* __restrict__ step_scalars,
                                                          const uint8_t* __restrict__ decays, float b1, float b2, float omb1, float omb2, float eps,
                                                          float clipnorm, float grad_scale, const int* __restrict__ skip_flag) {
    if (skip_flag != nullptr && *skip_flag != 0) return;      // w, m and v all stay put while the guard is up
    const int64_t t = slab_tensor[blockIdx.x];
    const int64_t off = (blockIdx.x - slab_first[t]) * (int64_t)SLAB;
    float* w = reinterpret_cast<float*>(ptrs[4 * t + 0]);
    const float* g = reinterpret_cast<const float*>(ptrs[4 * t + 1]);
    float* m = reinterpret_cast<float*>(ptrs[4 * t + 2]);
    float* v = reinterpret_cast<float*>(ptrs[4 * t + 3]);
    const int64_t n = sizes[t];
    AdamConsts c;
    c.lr_t = step_scalars[0]; c.wd_t = step_scalars[1];
    c.b1 = b1; c.b2 = b2; c.omb1 = omb1; c.omb2 = omb2; c.eps = eps;
    c.decay = decays == nullptr || decays[t] != 0;
    c.scale = grad_scale;
    if (clipnorm > 0.f) {
        const float nrm = norms[t] * fabsf(grad_scale);
        if (nrm > clipnorm) c.scale *= clipnorm / nrm;
    }
    const bool aligned = ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    const int64_t end = min(n, off + SLAB), nq = aligned ? (end - off) >> 2 : 0;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(g + off);
    f32x4* m4 = reinterpret_cast<f32x4*>(m + off);
    f32x4* v4 = reinterpret_cast<f32x4*>(v + off);
    f32x4* w4 = reinterpret_cast<f32x4*>(w + off);
    for (int64_t q = threadIdx.x; q < nq; q += 256) {
        const f32x4 gq = g4[q];
        f32x4 mq = m4[q], vq = v4[q], wq = w4[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float wi = wq[e], mi = mq[e], vi = vq[e];
            adamw_elem(c, gq[e], wi, mi, vi);
            wq[e] = wi; mq[e] = mi; vq[e] = vi;
        }
        m4[q] = mq; v4[q] = vq; w4[q] = wq;
    }
    for (int64_t i = off + 4 * nq + threadIdx.x; i < end; i += 256) {
        float wi = w[i], mi = m[i], vi = v[i];
        adamw_elem(c, g[i], wi, mi, vi);
        w[i] = wi; m[i] = mi; v[i] = vi;
    }
}

}  // namespace

// The slab table (slab_tensor[nslabs], slab_first[ntensors+1]) is built once by the host and
// lives on the device next to ptrs/sizes; partial: nslabs floats; norms: ntensors floats.
extern "C" int bdetr_sgd_slab_elems(void) { return SLAB; }

extern "C" int bdetr_sgd_nesterov_clipnorm(const uint64_t* ptrs, const int64_t* sizes, int ntensors,
                                           const int64_t* slab_tensor, const int64_t* slab_first, int nslabs,
                                           float* partial, float* norms, const float* lr, float momentum,
                                           float clipnorm, float grad_scale, int* skip_flag, void* stream) {
    BDETR_CHECK_ARG(ptrs && sizes && slab_tensor && slab_first && partial && norms && lr && ntensors > 0 && nslabs > 0,
                    "bdetr_sgd_nesterov_clipnorm: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    // (the norm pass reads the gradients the apply pass reads again: it takes the hint of the reductions, not the optimizer's)
    STREAM_DISPATCH(stream_on(STREAM_REDUCE), NT,
                    hipLaunchKernelGGL(sqnorm_kernel<NT>, dim3(nslabs), dim3(256), 0, st, ptrs, sizes, slab_tensor, slab_first, partial, 3));
    hipLaunchKernelGGL(norm_final_kernel, dim3((ntensors + 255) / 256), dim3(256), 0, st, partial, slab_first, ntensors, norms, skip_flag);
    STREAM_DISPATCH(stream_on(STREAM_OPTIM), NT, STREAM_DISPATCH(stream_on(STREAM_MOM_STORE), NTS,
                    hipLaunchKernelGGL((sgd_apply_kernel<NT, NTS>), dim3(nslabs), dim3(256), 0, st, ptrs, sizes, slab_tensor, slab_first, norms, lr, momentum, clipnorm, grad_scale, skip_flag)));
    return bdetr_launch_status("sgd_nesterov_clipnorm");
}

// AdamW / Adam: same tables and workspaces, rows of 4 pointers {w, g, m, v}; the two norm kernels are the ones above.
extern "C" int bdetr_adamw_clipnorm(const uint64_t* ptrs, const int64_t* sizes, int ntensors,
                                    const int64_t* slab_tensor, const int64_t* slab_first, int nslabs,
                                    float* partial, float* norms, const float* step_scalars, const uint8_t* decays,
                                    float beta1, float beta2, float one_minus_beta1, float one_minus_beta2, float epsilon,
                                    float clipnorm, float grad_scale, int* skip_flag, void* stream) {
    BDETR_CHECK_ARG(ptrs && sizes && slab_tensor && slab_first && partial && norms && step_scalars && ntensors > 0 && nslabs > 0,
                    "bdetr_adamw_clipnorm: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    STREAM_DISPATCH(stream_on(STREAM_REDUCE), NT,
                    hipLaunchKernelGGL(sqnorm_kernel<NT>, dim3(nslabs), dim3(256), 0, st, ptrs, sizes, slab_tensor, slab_first, partial, 4));
    hipLaunchKernelGGL(norm_final_kernel, dim3((ntensors + 255) / 256), dim3(256), 0, st, partial, slab_first, ntensors, norms, skip_flag);
    hipLaunchKernelGGL(adamw_apply_kernel, dim3(nslabs), dim3(256), 0, st, ptrs, sizes, slab_tensor, slab_first, norms, step_scalars, decays,
                       beta1, beta2, one_minus_beta1, one_minus_beta2, epsilon, clipnorm, grad_scale, skip_flag);
    return bdetr_launch_status("adamw_clipnorm");
}
