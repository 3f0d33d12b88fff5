// roi_head.hip -- the pooling of ResNetRoIHead (head_helper.py:103-118) over the channels-last token stream:
//     pooled[k, c] = max over bins of RoIAlign(mean_t x[b_k, t, :, :, c])
// AvgPool3d([T,1,1]) -> ROIAlign(resolution, 1/scale_factor, sampling_ratio=0, aligned) -> MaxPool2d(resolution), without the
// [B,C,T,H,W] transpose and without the [K, PH*PW, C] RoIAlign output: the bins of a box are reduced to a running max as
// they are sampled.  Geometry is roi_geometry.h, the same code as roi_align.hip (bit-exact with focus_roi_align_indices).
//
// forward   two launches.  (1) the temporal mean into an fp32 workspace [B, H*W, C]: x is read exactly once, summed over t in
//           order and divided by T.  (2) one workgroup per (box, 64 channels): 16 lanes x 4 channels times 16 bin slices;
//           every thread samples the bins slice, slice + 16, ... from the mean (L2-resident: 16 x 49 x 768 x 4 B = 2.4 MB
//           at the AVA shape) with the association of roi_fwd_kernel, keeps (max, lowest bin), and the 16 slices meet in LDS.
// backward  one launch, no atomics: one workgroup per (image, CS channels) owns its [H*W, CS] slab of d(mean) in LDS.
//           Lane c walks the boxes of its image in index order and adds the bilinear weights of bin arg[k, c] into column c
//           of the slab (no two lanes share a column), then the whole workgroup writes slab / T to all T frames of dx.
//           Every patch row of every image is written; the order of the sums is fixed, so two runs are bit-equal.
#include "focus_common.h"
// The geometry, the weights and every sum below are rounded operation by operation, as oracle/roi_align_ref.c and
// tests/roi_head_ref.py do: hipcc's __f*_rn intrinsics do not keep it from fusing start + p*bin into one fma (measured: the x
// of one bin one ulp off, the weight lx = 0.086 of its far neighbour off by 45 u), the rg_* operators of the strict form do.
#define ROI_GEOMETRY_STRICT
#include "roi_geometry.h"
#include <climits>

namespace {

constexpr int RH_MAX_T = 1024, RH_MAX_BINS = 1024, RH_MAX_HW = 512, RH_MAX_N = 65535;

// the batch index of a box: an integer in [0, B), else -1 (the box then reads and writes nothing)
__device__ __forceinline__ int roi_batch(const float* roi5, int B) {
    const float bf = roi5[0];
    if (!(bf >= 0.f && bf < (float)B) || bf != floorf(bf)) return -1;
    return (int)bf;
}

template <typename T>
__global__ __launch_bounds__(256) void roi_head_mean_kernel(const T* __restrict__ x, int64_t bstride,
                                                            float* __restrict__ m, int B, int Tn, int HW, int C) {
    const int cq = C >> 2;
    const int64_t n = (int64_t)B * HW * cq;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % cq) * 4;
        const int64_t cell = (i / cq) % HW, b = i / ((int64_t)cq * HW);
        const T* p = x + b * bstride + cell * C + c;
        f4 s = {0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < Tn; ++t) {
            const f4 v = ld4<T>(p + (int64_t)t * HW * C);
            s.x = rg_add(s.x, v.x); s.y = rg_add(s.y, v.y); s.z = rg_add(s.z, v.z); s.w = rg_add(s.w, v.w);
        }
        const float d = (float)Tn;
        s.x = rg_div(s.x, d); s.y = rg_div(s.y, d); s.z = rg_div(s.z, d); s.w = rg_div(s.w, d);
        st4<float>(m + (b * HW + cell) * C + c, s);
    }
}

__device__ __forceinline__ void keep_max(float v, int bin, float& best, int& arg) {
    if (v > best || (v == best && bin < arg)) { best = v; arg = bin; }
}

// grid (ceil(C / 64), K), 256 threads: thread = (bin slice = tid / 16, channel quad = tid % 16)
template <typename T>
__global__ __launch_bounds__(256) void roi_head_pool_kernel(const float* __restrict__ m, const float* __restrict__ rois,
                                                            T* __restrict__ pooled, int32_t* __restrict__ arg, int B,
                                                            int H, int W, int C, int PH, int PW, float scale, int sr,
                                                            int aligned) {
    __shared__ float sv[16][64];
    __shared__ int sa[16][64];
    const int k = blockIdx.y, c0 = blockIdx.x * 64;
    const int q = threadIdx.x & 15, slice = threadIdx.x >> 4, c = c0 + q * 4;
    const int b = roi_batch(rois + 5 * k, B);                                     // block-uniform
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    int barg[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
    if (b >= 0 && c < C) {
        const Geom g = roi_geometry(rois + 5 * k + 1, scale, PH, PW, sr, aligned);
        const float* img = m + (int64_t)b * H * W * C + c;
        const int bins = PH * PW;
        for (int bin = slice; bin < bins; bin += 16) {
            const int ph = bin / PW, pw = bin % PW;
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int iy = 0; iy < g.grid_h; ++iy) {
                const float y = sample_coord(g.y1, ph, g.bin_h, iy, g.grid_h);
                for (int ix = 0; ix < g.grid_w; ++ix) {
                    const float x = sample_coord(g.x1, pw, g.bin_w, ix, g.grid_w);
                    const Nbr n = locate(y, x, H, W);
                    if (n.y_low < 0) continue;
                    const f4 a = ld4<float>(img + (int64_t)(n.y_low * W + n.x_low) * C);
                    const f4 bb = ld4<float>(img + (int64_t)(n.y_low * W + n.x_high) * C);
                    const f4 cc = ld4<float>(img + (int64_t)(n.y_high * W + n.x_low) * C);
                    const f4 dd = ld4<float>(img + (int64_t)(n.y_high * W + n.x_high) * C);
                    // the association of roi_fwd_kernel and the oracle: acc += w1*a + w2*b + w3*c + w4*d
                    acc.x = rg_add(acc.x, rg_add(rg_add(rg_add(rg_mul(n.w1, a.x), rg_mul(n.w2, bb.x)), rg_mul(n.w3, cc.x)), rg_mul(n.w4, dd.x)));
                    acc.y = rg_add(acc.y, rg_add(rg_add(rg_add(rg_mul(n.w1, a.y), rg_mul(n.w2, bb.y)), rg_mul(n.w3, cc.y)), rg_mul(n.w4, dd.y)));
                    acc.z = rg_add(acc.z, rg_add(rg_add(rg_add(rg_mul(n.w1, a.z), rg_mul(n.w2, bb.z)), rg_mul(n.w3, cc.z)), rg_mul(n.w4, dd.z)));
                    acc.w = rg_add(acc.w, rg_add(rg_add(rg_add(rg_mul(n.w1, a.w), rg_mul(n.w2, bb.w)), rg_mul(n.w3, cc.w)), rg_mul(n.w4, dd.w)));
                }
            }
            keep_max(rg_div(acc.x, g.count), bin, best[0], barg[0]);
            keep_max(rg_div(acc.y, g.count), bin, best[1], barg[1]);
            keep_max(rg_div(acc.z, g.count), bin, best[2], barg[2]);
            keep_max(rg_div(acc.w, g.count), bin, best[3], barg[3]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { sv[slice][q * 4 + j] = best[j]; sa[slice][q * 4 + j] = barg[j]; }
    __syncthreads();
    const int ch = c0 + threadIdx.x;
    if (threadIdx.x < 64 && ch < C) {
        float v = 0.f;
        int a = 0;
        if (b >= 0) {
            v = sv[0][threadIdx.x]; a = sa[0][threadIdx.x];                        // slice 0 always holds bin 0
            for (int s = 1; s < 16; ++s) keep_max(sv[s][threadIdx.x], sa[s][threadIdx.x], v, a);
        }
        st<T>(pooled + (int64_t)k * C + ch, v);
        arg[(int64_t)k * C + ch] = a;
    }
}

// grid (ceil(C / CS), B), 256 threads, dynamic LDS [H*W][CS] fp32
template <typename T, int CS>
__global__ __launch_bounds__(256) void roi_head_bwd_kernel(const T* __restrict__ dpooled, const int32_t* __restrict__ arg,
                                                           const float* __restrict__ rois, T* __restrict__ dx,
                                                           int64_t bstride, int B, int Tn, int H, int W, int C, int K,
                                                           int PH, int PW, float scale, int sr, int aligned) {
    extern __shared__ __attribute__((aligned(16))) float slab[];
    const int b = blockIdx.y, c0 = blockIdx.x * CS, HW = H * W;
    for (int i = threadIdx.x; i < HW * CS; i += 256) slab[i] = 0.f;
    __syncthreads();
    const int ch = c0 + threadIdx.x;
    if (threadIdx.x < CS && ch < C) {
        float* col = slab + threadIdx.x;
        const int bins = PH * PW;
        for (int k = 0; k < K; ++k) {
            if (roi_batch(rois + 5 * k, B) != b) continue;                         // wave-uniform
            const Geom g = roi_geometry(rois + 5 * k + 1, scale, PH, PW, sr, aligned);
            if (g.grid_h <= 0 || g.grid_w <= 0) continue;
            const int a = arg[(int64_t)k * C + ch];
            if (a < 0 || a >= bins) continue;
            const int ph = a / PW, pw = a % PW;
            const float gv = rg_div(ld<T>(dpooled + (int64_t)k * C + ch), g.count);
            for (int iy = 0; iy < g.grid_h; ++iy) {
                const float y = sample_coord(g.y1, ph, g.bin_h, iy, g.grid_h);
                for (int ix = 0; ix < g.grid_w; ++ix) {
                    const float x = sample_coord(g.x1, pw, g.bin_w, ix, g.grid_w);
                    const Nbr n = locate(y, x, H, W);
                    if (n.y_low < 0) continue;
                    float* p1 = col + (n.y_low * W + n.x_low) * CS;
                    float* p2 = col + (n.y_low * W + n.x_high) * CS;
                    float* p3 = col + (n.y_high * W + n.x_low) * CS;
                    float* p4 = col + (n.y_high * W + n.x_high) * CS;
                    *p1 = rg_add(*p1, rg_mul(gv, n.w1));                     // in this order: p1..p4 may coincide at the edges
                    *p2 = rg_add(*p2, rg_mul(gv, n.w2));
                    *p3 = rg_add(*p3, rg_mul(gv, n.w3));
                    *p4 = rg_add(*p4, rg_mul(gv, n.w4));
                }
            }
        }
    }
    __syncthreads();
    constexpr int QS = CS / 4, RS = 256 / QS;                                       // channel quads, rows per sweep
    const int q = threadIdx.x % QS, r0 = threadIdx.x / QS, c = c0 + q * 4;
    if (c >= C) return;
    const float d = (float)Tn;
    T* out = dx + (int64_t)b * bstride + c;
    for (int row = r0; row < Tn * HW; row += RS) {
        const float4 v = *reinterpret_cast<const float4*>(slab + (row % HW) * CS + q * 4);
        st4<T>(out + (int64_t)row * C, {rg_div(v.x, d), rg_div(v.y, d), rg_div(v.z, d), rg_div(v.w, d)});
    }
}

int roi_head_check(const void* x, int64_t bstride, int B, int T, int H, int W, int C, int K, int PH, int PW, int dtype) {
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || C <= 0 || K < 0 || PH <= 0 || PW <= 0) return FOCUS_ERR_SHAPE;
    if (T > RH_MAX_T || (int64_t)PH * PW > RH_MAX_BINS || (int64_t)H * W > RH_MAX_HW || K > RH_MAX_N || B > RH_MAX_N)
        return FOCUS_ERR_SHAPE;
    if (bstride < (int64_t)T * H * W * C) return FOCUS_ERR_SHAPE;
    if ((C & 3) || (bstride & 3) || !focus_aligned(x, 4 * focus_esize(dtype))) return FOCUS_ERR_ALIGN;
    return FOCUS_OK;
}

}  // namespace

extern "C" size_t focus_roi_head_workspace_bytes(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return 0;
    return (size_t)B * H * W * C * sizeof(float);
}

extern "C" int focus_roi_head_fwd(const void* x, int64_t batch_stride, const float* rois, void* pooled, int32_t* arg,
                                  void* ws, size_t ws_bytes, int B, int T, int H, int W, int C, int K, int PH, int PW,
                                  float spatial_scale, int sampling_ratio, int aligned, int dtype, void* stream) {
    const int st_ = roi_head_check(x, batch_stride, B, T, H, W, C, K, PH, PW, dtype);
    if (st_ != FOCUS_OK) return st_;
    if (K == 0) return FOCUS_OK;
    if (!x || !rois || !pooled || !arg || !ws) return FOCUS_ERR_NULL;
    if (ws_bytes < focus_roi_head_workspace_bytes(B, H, W, C) || !focus_aligned(ws, 16)) return FOCUS_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* m = static_cast<float*>(ws);
    const int64_t n4 = (int64_t)B * H * W * (C >> 2);
    const int mgrid = (int)(cdiv64(n4, 256) < 2048 ? cdiv64(n4, 256) : 2048);
    dim3 grid((C + 63) / 64, K);
    if (dtype == FOCUS_BF16) {
        hipLaunchKernelGGL((roi_head_mean_kernel<bf16_t>), dim3(mgrid), dim3(256), 0, s, (const bf16_t*)x, batch_stride, m,
                           B, T, H * W, C);
        hipLaunchKernelGGL((roi_head_pool_kernel<bf16_t>), grid, dim3(256), 0, s, m, rois, (bf16_t*)pooled, arg, B, H, W, C,
                           PH, PW, spatial_scale, sampling_ratio, aligned);
    } else {
        hipLaunchKernelGGL((roi_head_mean_kernel<float>), dim3(mgrid), dim3(256), 0, s, (const float*)x, batch_stride, m, B,
                           T, H * W, C);
        hipLaunchKernelGGL((roi_head_pool_kernel<float>), grid, dim3(256), 0, s, m, rois, (float*)pooled, arg, B, H, W, C,
                           PH, PW, spatial_scale, sampling_ratio, aligned);
    }
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_roi_head_bwd(const void* dpooled, const int32_t* arg, const float* rois, void* dx,
                                  int64_t batch_stride, int B, int T, int H, int W, int C, int K, int PH, int PW,
                                  float spatial_scale, int sampling_ratio, int aligned, int dtype, void* stream) {
    const int st_ = roi_head_check(dx, batch_stride, B, T, H, W, C, K, PH, PW, dtype);
    if (st_ != FOCUS_OK) return st_;
    if (!dx || (K > 0 && (!dpooled || !arg || !rois))) return FOCUS_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const int HW = H * W;
    const int cs = HW <= 256 ? 64 : 32;                       // the slab [H*W][cs] fp32 stays within 64 KiB of LDS
    const size_t lds = (size_t)HW * cs * sizeof(float);
    dim3 grid((C + cs - 1) / cs, B);
#define ROI_HEAD_BWD(TT, CS) do { \
        auto kern = roi_head_bwd_kernel<TT, CS>; \
        if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) \
            return FOCUS_ERR_LAUNCH; \
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, (const TT*)dpooled, arg, rois, (TT*)dx, batch_stride, B, T, H, W, C, \
                           K, PH, PW, spatial_scale, sampling_ratio, aligned); } while (0)
    if (dtype == FOCUS_BF16) { if (cs == 64) ROI_HEAD_BWD(bf16_t, 64); else ROI_HEAD_BWD(bf16_t, 32); }
    else { if (cs == 64) ROI_HEAD_BWD(float, 64); else ROI_HEAD_BWD(float, 32); }
#undef ROI_HEAD_BWD
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
