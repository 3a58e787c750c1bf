// Valid image regions -> attention key masks over the feature tokens (include/bdetr.h K35).
//
// One thread per token, one plain byte store each.  The regions are read from HBM by the kernel, so a captured step that is
// replayed with other regions in its static input buffer makes the mask of THOSE regions.
#include "common.h"

namespace {

constexpr int TKM_BLOCK = 256;
constexpr int TKM_MAX_DIM = 1 << 20;      // h, w, r, c: every product of the rule then stays below 2^54

// keep iff 2 n lo <= (2 idx + 1) size < 2 n (lo + len), in int64 (lo + len of two int32 cannot overflow it)
__device__ __forceinline__ bool centre_inside(int64_t idx, int64_t size, int64_t n, int64_t lo, int64_t len) {
    const int64_t centre = (2 * idx + 1) * size;
    return 2 * n * lo <= centre && centre < 2 * n * (lo + len);
}

__global__ __launch_bounds__(TKM_BLOCK) void token_key_mask_kernel(const int32_t* __restrict__ region, int h, int w, int r, int c,
                                                                   uint8_t* __restrict__ mask) {
    const int T = r * c;
    const int t = (int)blockIdx.x * TKM_BLOCK + (int)threadIdx.x;
    if (t >= T) return;
    const int b = (int)blockIdx.y;
    const int32_t* g = region + 4 * (int64_t)b;
    const int64_t top = g[0], left = g[1], height = g[2], width = g[3];
    const int i = t / c, j = t - i * c;
    const bool keep = centre_inside(i, h, r, top, height) && centre_inside(j, w, c, left, width);
    mask[(int64_t)b * T + t] = keep ? 1 : 0;
}

}  // namespace

extern "C" int bdetr_token_key_mask(const int32_t* region, int B, int h, int w, int r, int c, uint8_t* mask, void* stream) {
    BDETR_CHECK_ARG(region && mask, "bdetr_token_key_mask: null pointer");
    BDETR_CHECK_ARG(B > 0 && B <= 65535, "bdetr_token_key_mask: B=%d must be in [1, 65535]", B);
    BDETR_CHECK_ARG(h > 0 && w > 0 && r > 0 && c > 0 && h <= TKM_MAX_DIM && w <= TKM_MAX_DIM && r <= TKM_MAX_DIM && c <= TKM_MAX_DIM,
                    "bdetr_token_key_mask: h=%d w=%d r=%d c=%d must be in [1, %d]", h, w, r, c, TKM_MAX_DIM);
    BDETR_CHECK_ARG((int64_t)r * c <= 0x7fffffff - TKM_BLOCK, "bdetr_token_key_mask: %lld tokens are too many", (long long)r * c);
    const dim3 grid((unsigned)cdiv64((int64_t)r * c, TKM_BLOCK), (unsigned)B);
    hipLaunchKernelGGL(token_key_mask_kernel, grid, dim3(TKM_BLOCK), 0, (hipStream_t)stream, region, h, w, r, c, mask);
    return bdetr_launch_status("token_key_mask");
}
