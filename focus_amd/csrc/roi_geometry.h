// roi_geometry.h -- the geometry of RoIAlign shared by roi_align.hip and roi_head.hip.
// Follows oracle/roi_align_ref.c operation by operation in fp32, so that sampling-grid sizes and neighbour indices agree
// with the oracle (focus_roi_align_indices exports them); see rg_* below for what "operation by operation" takes.
#pragma once
#include "focus_common.h"

// rg_add / rg_sub / rg_mul / rg_div: the arithmetic of the geometry.  By default hipcc's __f*_rn intrinsics, as roi_align.hip
// has always used them.  They are plain operators compiled under -ffp-contract=fast, so after inlining hipcc may still fuse a
// product into the sum that follows it (start + p*bin becomes one fma, one rounding less than the oracle: a coordinate can
// land one ulp off).  A file that defines ROI_GEOMETRY_STRICT before including this header gets operators compiled with
// contraction off: one rounding per operation, exactly oracle/roi_align_ref.c.
#ifdef ROI_GEOMETRY_STRICT
namespace {
__device__ __forceinline__ float rg_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rg_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float rg_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float rg_div(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
}  // namespace
#else
#define rg_add __fadd_rn
#define rg_sub __fsub_rn
#define rg_mul __fmul_rn
#define rg_div __fdiv_rn
#endif

namespace {

struct Geom { float y1, x1, bin_h, bin_w; int grid_h, grid_w; float count; };
struct Nbr { int y_low, x_low, y_high, x_high; float w1, w2, w3, w4; };

__device__ __forceinline__ Geom roi_geometry(const float* roi, float scale, int PH, int PW, int sampling_ratio,
                                             int aligned) {
    Geom g;
    const float off = aligned ? 0.5f : 0.0f;
    g.x1 = rg_sub(rg_mul(roi[0], scale), off);
    g.y1 = rg_sub(rg_mul(roi[1], scale), off);
    const float x2 = rg_sub(rg_mul(roi[2], scale), off);
    const float y2 = rg_sub(rg_mul(roi[3], scale), off);
    float rw = rg_sub(x2, g.x1), rh = rg_sub(y2, g.y1);
    if (!aligned) { if (rw < 1.0f) rw = 1.0f; if (rh < 1.0f) rh = 1.0f; }
    g.bin_h = rg_div(rh, (float)PH);
    g.bin_w = rg_div(rw, (float)PW);
    g.grid_h = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rg_div(rh, (float)PH));
    g.grid_w = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rg_div(rw, (float)PW));
    const int c = g.grid_h * g.grid_w;
    g.count = (float)(c > 1 ? c : 1);
    return g;
}
__device__ __forceinline__ float sample_coord(float start, int p, float bin, int i, int grid) {
    // start + p*bin + (i + 0.5)*bin/grid, evaluated left to right as in the oracle
    return rg_add(rg_add(start, rg_mul((float)p, bin)),
                     rg_div(rg_mul(rg_add((float)i, 0.5f), bin), (float)grid));
}
__device__ __forceinline__ Nbr locate(float y, float x, int H, int W) {
    Nbr n;
    if (y < -1.0f || y > (float)H || x < -1.0f || x > (float)W) {
        n.y_low = n.x_low = n.y_high = n.x_high = -1;
        n.w1 = n.w2 = n.w3 = n.w4 = 0.f;
        return n;
    }
    if (y <= 0.f) y = 0.f;
    if (x <= 0.f) x = 0.f;
    n.y_low = (int)y;
    n.x_low = (int)x;
    if (n.y_low >= H - 1) { n.y_high = n.y_low = H - 1; y = (float)n.y_low; } else n.y_high = n.y_low + 1;
    if (n.x_low >= W - 1) { n.x_high = n.x_low = W - 1; x = (float)n.x_low; } else n.x_high = n.x_low + 1;
    const float ly = rg_sub(y, (float)n.y_low), lx = rg_sub(x, (float)n.x_low);
    const float hy = rg_sub(1.0f, ly), hx = rg_sub(1.0f, lx);
    n.w1 = rg_mul(hy, hx); n.w2 = rg_mul(hy, lx); n.w3 = rg_mul(ly, hx); n.w4 = rg_mul(ly, lx);
    return n;
}

}  // namespace
