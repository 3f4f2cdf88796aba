// What the bilinear resize kernels (gt_resize.hip) and the fused conv0 + resize kernels (gt_convresize.hip) share: the source
// index / weight rule of one output coordinate (torch's align_corners=True) and the host-side scale.  gfx950 only.
#pragma once
#include "gt_common.h"

namespace gt {

struct Axis {               // source index / weights of one output coordinate (torch's align_corners rule)
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Axis axis_of(int o, float scale, int ni) {
    // The reference rounds scale*o to fp32 before taking floor and fraction.  Letting the compiler
    // contract `scale*o - i0` into one fma changes the weights by up to 1 ulp of src (~1e-5 relative at
    // o ~ 100), so contraction is switched off for this function.
#pragma clang fp contract(off)
    const float src = scale * (float)o;
    int i0 = (int)src;
    i0 = min(i0, ni - 1);
    Axis a;
    a.i0 = i0;
    a.i1 = i0 + (i0 < ni - 1 ? 1 : 0);
    a.l1 = src - (float)i0;
    a.l0 = 1.f - a.l1;
    return a;
}

static inline float scale_of(int ni, int no) { return (no > 1) ? (float)(ni - 1) / (float)(no - 1) : 0.f; }

}  // namespace gt
