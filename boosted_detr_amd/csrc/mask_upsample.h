// mask_upsample.h - the value of an image pixel under the mask head's G x G logits on gfx950 (K19's rule, include/bdetr.h),
// written once: bilinear with half-pixel centres, the axis rule in integers and the value in fp64 with every product and every
// sum rounded on its own (no FMA), so NumPy reproduces it bit for bit.  Two kernels call it:
//   maskimage.hip      mask_upsample_bits_kernel (K19)  one query's mask: value > 0
//   panopticmerge.hip  panoptic_merge_kernel (K24)      the kept query with the largest value > 0
// so the merged mask of a single kept query is K19's by construction.  Their x-axis tables and their loops are their own.
//
// Exactness does not depend on who includes this: contraction is off from here on (build.py also passes -ffp-contract=off for
// the two files).
#pragma once
#pragma clang fp contract(off)
#include "common.h"

namespace maskup {

constexpr int MAX_G = 32;                 // logit grid cells per side (K18's limit)

struct axis {
    int ia, ib;
    double t;
};

// target pixel p of n along an axis of G source cells: the two source cells and the weight of the second one
__device__ __forceinline__ axis axis_rule(int p, int n, int G) {
    const int num = (2 * p + 1) * G - n, D = 2 * n;
    const int i0 = num >= 0 ? num / D : -((D - 1 - num) / D);      // floor division: -1 for every negative num (|num| < D)
    const int r = num - i0 * D;
    axis a;
    a.ia = min(max(i0, 0), G - 1);
    a.ib = min(max(i0 + 1, 0), G - 1);
    a.t = (double)r / (double)D;
    return a;
}

// the logits of rows ya, yb at columns xa, xb; tx, ty the weights of xb, yb and ux = 1 - tx, uy = 1 - ty
__device__ __forceinline__ double bilinear(double ux, double tx, double uy, double ty, float l_aa, float l_ab, float l_ba, float l_bb) {
    const double top = ux * (double)l_aa + tx * (double)l_ab;
    const double bot = ux * (double)l_ba + tx * (double)l_bb;
    return uy * top + ty * bot;
}

}  // namespace maskup
