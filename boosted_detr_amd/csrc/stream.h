// stream.h - cache policy of operands that a launch touches exactly once ("stream-once operands").
//
// ld_stream<NT>(p) / st_stream<NT>(p, v): with NT the access carries the non-temporal hint (__builtin_nontemporal_load / _store; on gfx950
// `global_load_dwordx4 ... nt` / `global_store_dwordx4 ... nt`: the load bypasses the CU's L1 and is served by L2, the line is marked for
// early eviction), without it it is the plain access the kernels had before.  NT is a template parameter of the kernel, chosen by
// the host at launch from bdetr_stream_policy(): no run-time branch in any loop, and policy 0 launches the instantiation whose
// accesses are the plain ones.  A hint changes no value: every kernel computes the same bits under every policy.
#pragma once
#include "common.h"

// operand classes a policy bit switches (BDETR_STREAM_POLICY = sum of the bits; 0 = every access default)
enum {
    STREAM_APPLY = 1,         // bn_apply_p16_kernel, bn_bwd_apply_p16_kernel: activation, residual, gradient and mask loads at their last use
    STREAM_REDUCE = 2,        // column reductions (colreduce2_kernel) and the gradient-norm pass: loads of tensors the pass that follows reads again
    STREAM_OPTIM = 4,         // optimizer step and weight pack: gradient, momentum and weight loads
    STREAM_GEMM_EPI = 8,      // float4 epilogue of the fused 1x1 backward-data (masked accumulate): old gradient and its mask
    STREAM_MOM_STORE = 16,    // the optimizer's momentum store (next read one step away)
    STREAM_APPLY_OTHER = 32,  // the other element-wise passes: fp32 bn_apply / bn_bwd_apply, the stem pair, relu_mask_apply
    STREAM_ALL = 63,
    // In force when BDETR_STREAM_POLICY is unset: the one class that won in the training step (profiles/stream_policy_2026-10-20.txt:
    // +1.2 % images/s; every other class measured equal or slower, in the step and kernel by kernel).
    STREAM_DEFAULT = STREAM_APPLY
};

// the policy of this process: BDETR_STREAM_POLICY, read once (common.cpp)
int bdetr_stream_policy_bits();
static inline bool stream_on(int bit) { return (bdetr_stream_policy_bits() & bit) != 0; }

template <bool NT, class T>
__device__ __forceinline__ T ld_stream(const T* p) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "ld_stream: 4-, 8- and 16-byte types");
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT, class T>
__device__ __forceinline__ void st_stream(T* p, const T v) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16, "st_stream: 4-, 8- and 16-byte types");
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}
// float4 number i of a float tensor
template <bool NT>
__device__ __forceinline__ f32x4 ld_stream4(const float* base, int64_t i) { return ld_stream<NT>(reinterpret_cast<const f32x4*>(base) + i); }

// launch `expr` with NT bound to a compile-time bool: STREAM_DISPATCH(stream_on(STREAM_APPLY), NT, hipLaunchKernelGGL((k<NT>), ...))
#define STREAM_DISPATCH(cond, NT, ...)                                     \
    do {                                                                   \
        if (cond) { constexpr bool NT = true; __VA_ARGS__; }               \
        else { constexpr bool NT = false; __VA_ARGS__; }                   \
    } while (0)
