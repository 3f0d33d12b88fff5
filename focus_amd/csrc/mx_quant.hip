// mx_quant.hip -- MX e4m3 activations: bf16 X [rows, cols] -> OCP e4m3 codes [rows, cols] + one E8M0 scale byte per
// block of 32 consecutive elements of a row (the A operand of gemm_mx_fp8.hip).  For a block with largest magnitude amax:
//   e     = the smallest integer with amax <= 448 * 2^e, clamped to [-127, 127] (all-zero block: -127).  From the bits of
//           amax = 1.m x 2^E:  e = E - 8 + (m > 0.75).  A ceiling rule: no element saturates (the OCP MX v1.0 text
//           floors, which clips the top of a block to 448).
//   scale = e + 127 (0xFF for a block holding a NaN or an Inf; its codes are then unspecified: here NaN codes)
//   code  = RNE_e4m3(x * 2^-e), the product in fp32 (exact wherever the code is not zero)
// One pass: every thread reads 8 bf16 (16 B) once and writes their 8 codes; the 4 lanes of a block meet in two lane
// exchanges for amax.  tests/mx_ref.py is the numpy statement of the same rule, checked bit for bit.
#include "focus_common.h"

namespace {

__device__ __forceinline__ uint32_t pack4_e4m3(float a, float b, float c, float d) {
    int v = 0;
    v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, v, false);      // bytes 0, 1
    v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);       // bytes 2, 3
    return (uint32_t)v;
}

__device__ __forceinline__ uint32_t amax2(uint32_t w) { return max(w & 0x7fffu, (w >> 16) & 0x7fffu); }

// thread t: row t / c8, elements 8 (t % c8) .. +7.  c8 = cols / 8 is a multiple of 4, so an aligned quad of lanes is one
// 32-element block of one row (and a quad past the end is wholly past it)
__global__ __launch_bounds__(256) void mx_quant_kernel(const bf16_t* __restrict__ x, int64_t ldx, uint32_t total, uint32_t c8,
                                                       uint8_t* __restrict__ codes, int64_t ldc, uint8_t* __restrict__ scales,
                                                       int64_t lds) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const bool live = t < total;
    const uint32_t r = live ? t / c8 : 0u, c = live ? t - r * c8 : 0u;
    uint4 v = {0u, 0u, 0u, 0u};
    if (live) v = *reinterpret_cast<const uint4*>(x + (int64_t)r * ldx + c * 8);
    // |x| as bf16 bits: on non-negative values the integer order is the float order, and a NaN (above 0x7F80) wins the
    // max instead of being dropped as fmaxf would drop it
    uint32_t a = max(max(amax2(v.x), amax2(v.y)), max(amax2(v.z), amax2(v.w)));
    a = max(a, (uint32_t)__shfl_xor((int)a, 1));
    a = max(a, (uint32_t)__shfl_xor((int)a, 2));
    if (!live) return;
    int e = (int)(a >> 7) - 127 - 8 + ((a & 0x7fu) > 0x60u ? 1 : 0);   // bf16 mantissa > 0.75 = 96 / 128
    e = min(max(e, -127), 127);
    const float inv = __uint_as_float((uint32_t)(127 - e) << 23);       // 2^-e (e <= 120 for every finite amax)
    const float f[8] = {__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u),
                        __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u),
                        __uint_as_float(v.z << 16), __uint_as_float(v.z & 0xffff0000u),
                        __uint_as_float(v.w << 16), __uint_as_float(v.w & 0xffff0000u)};
    uint2 o;
    o.x = pack4_e4m3(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
    o.y = pack4_e4m3(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
    const bool bad = a >= 0x7f80u;                                      // a NaN or an Inf in the block
    if (bad) o.x = o.y = 0x7f7f7f7fu;   // NaN codes beside the NaN scale: the block's products are NaN whatever reads them
    *reinterpret_cast<uint2*>(codes + (int64_t)r * ldc + c * 8) = o;
    if ((c & 3u) == 0u) scales[(int64_t)r * lds + (c >> 2)] = bad ? (uint8_t)0xff : (uint8_t)(e + 127);
}

}  // namespace

extern "C" int focus_mx_quant(const void* x, int64_t ldx, int rows, int cols, int dtype, void* codes, int64_t ld_codes,
                              void* scales, int64_t ld_scales, void* stream) {
    if (!x || !codes || !scales) return FOCUS_ERR_NULL;
    if (dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (rows < 0 || cols <= 0 || (cols % 32) != 0 || ldx < cols || ld_codes < cols || ld_scales < cols / 32)
        return FOCUS_ERR_SHAPE;
    if ((int64_t)rows * (cols / 8) >= ((int64_t)1 << 31)) return FOCUS_ERR_SHAPE;
    if (!focus_aligned(x, 16) || (ldx & 7) || !focus_aligned(codes, 16) || (ld_codes & 15) || !focus_aligned(scales, 4) ||
        (ld_scales & 3))
        return FOCUS_ERR_ALIGN;
    if (rows == 0) return FOCUS_OK;
    const uint32_t c8 = (uint32_t)(cols / 8), total = (uint32_t)rows * c8;
    hipLaunchKernelGGL(mx_quant_kernel, dim3((total + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const bf16_t*>(x), ldx, total, c8, static_cast<uint8_t*>(codes), ld_codes,
                       static_cast<uint8_t*>(scales), ld_scales);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
