// clip_sample.hip -- decoded uint8 clips -> model inputs in one pass: crop, bilinear resize (align_corners=False), window,
// mirror, /255, mean/std normalisation, optional channel reversal and the cast to the model's dtype
// (datasets/utils.py:111-188, 319-336 and transform.py:42-272, 520-602 of the reference, for all three sampling modes).
//
// Work split: a thread owns RUN = 8 consecutive output x of one output row, for all three channels, so the y taps and
// weights are computed once per thread and each channel plane gets one (bf16) or two (fp32) 16-byte stores when the
// address allows it.  Threads run along x, then y; blockIdx.y is the frame, blockIdx.z the clip, so the descriptor is
// block-uniform.  The source is read byte by byte: an RGB row of W*3 bytes is in general not dword aligned.  The four
// taps of neighbouring pixels overlap and come out of the vector cache.  No LDS, no atomics, no workspace: every output
// element is written once by one thread from a fixed expression, so the same call gives the same bits.
#include "focus_common.h"

namespace {

constexpr int RUN = 8;
constexpr int THREADS = 256;

struct ClipNorm { float a[3], b[3]; };      // out = raw * a[c'] + b[c'],  a = 1 / (255 std),  b = -mean / std

template <typename T>
__global__ __launch_bounds__(THREADS) void clip_sample_kernel(const focus_clip_item* __restrict__ items, int out_h, int out_w,
                                                              T* __restrict__ out, int64_t sb, int64_t sc, int64_t sf,
                                                              ClipNorm nrm, int reverse) {
    const int runs = (out_w + RUN - 1) / RUN;
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= runs * out_h) return;
    const int y = idx / runs, xb = (idx - y * runs) * RUN;
    const int t = blockIdx.y, b = blockIdx.z;
    const focus_clip_item it = items[b];
    // memory safety only (the caller validates the rectangle): never read outside [0,H) x [0,W)
    const int sy0 = min(max(it.sy0, 0), it.H - 1), sx0 = min(max(it.sx0, 0), it.W - 1);
    const int sh = min(it.sh, it.H - sy0), sw = min(it.sw, it.W - sx0);
    if (it.H <= 0 || it.W <= 0 || sh <= 0 || sw <= 0 || it.rh <= 0 || it.rw <= 0) return;

    const float scale_y = (float)sh / (float)it.rh, scale_x = (float)sw / (float)it.rw;
    const float sy = fmaxf(((float)(y + it.oy0) + 0.5f) * scale_y - 0.5f, 0.0f);
    const int y0 = min((int)sy, sh - 1), y1 = min(y0 + 1, sh - 1);
    const float ly = sy - (float)y0;
    const uint8_t* frame = it.src + (int64_t)t * it.frame_stride + (int64_t)sx0 * 3;
    const uint8_t* row0 = frame + (int64_t)(sy0 + y0) * it.row_stride;
    const uint8_t* row1 = frame + (int64_t)(sy0 + y1) * it.row_stride;

    const int n = min(RUN, out_w - xb);
    float v[3][RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        if (j < n) {
            const int x = xb + j;
            const int xo = it.flip ? out_w - 1 - x : x;
            const float sx = fmaxf(((float)(xo + it.ox0) + 0.5f) * scale_x - 0.5f, 0.0f);
            const int x0 = min((int)sx, sw - 1), x1 = min(x0 + 1, sw - 1);
            const float lx = sx - (float)x0;
            const uint8_t *p00 = row0 + x0 * 3, *p01 = row0 + x1 * 3, *p10 = row1 + x0 * 3, *p11 = row1 + x1 * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float top = (float)p00[c] + lx * ((float)p01[c] - (float)p00[c]);      // byte differences are exact
                const float bot = (float)p10[c] + lx * ((float)p11[c] - (float)p10[c]);
                v[c][j] = top + ly * (bot - top);
            }
        } else {
            v[0][j] = v[1][j] = v[2][j] = 0.0f;
        }
    }

    T* orow = out + (int64_t)b * sb + (int64_t)t * sf + (int64_t)y * out_w + xb;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        // output channel c shows source channel c' = reverse ? 2 - c : c (selects, not a dynamic register index)
        const float a = reverse ? nrm.a[2 - c] : nrm.a[c], bb = reverse ? nrm.b[2 - c] : nrm.b[c];
        float o[RUN];
#pragma unroll
        for (int j = 0; j < RUN; ++j) o[j] = fmaf(reverse ? v[2 - c][j] : v[c][j], a, bb);
        T* p = orow + (int64_t)c * sc;
        if (n == RUN && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            st8<T>(p, o);
        } else {
#pragma unroll
            for (int j = 0; j < RUN; ++j)
                if (j < n) st<T>(p + j, o[j]);
        }
    }
}

}  // namespace

extern "C" int focus_clip_sample(const focus_clip_item* items, int n_clips, int T, int out_h, int out_w, void* out,
                                 int64_t sb, int64_t sc, int64_t st, const float* mean, const float* std, int reverse,
                                 int dtype, void* stream) {
    if (!items || !out || !mean || !std) return FOCUS_ERR_NULL;
    if (n_clips <= 0 || T <= 0) return FOCUS_OK;
    if (out_h <= 0 || out_w <= 0 || T > 65535 || n_clips > 65535) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    const int64_t work = (int64_t)((out_w + RUN - 1) / RUN) * out_h;
    if (work > (int64_t)0x7fffffff - THREADS) return FOCUS_ERR_SHAPE;
    ClipNorm nrm;
    for (int c = 0; c < 3; ++c) {
        nrm.a[c] = (float)(1.0 / (255.0 * (double)std[c]));
        nrm.b[c] = (float)(-(double)mean[c] / (double)std[c]);
    }
    const dim3 grid((unsigned)cdiv64(work, THREADS), (unsigned)T, (unsigned)n_clips);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        clip_sample_kernel<bf16_t><<<grid, THREADS, 0, s>>>(items, out_h, out_w, (bf16_t*)out, sb, sc, st, nrm, reverse ? 1 : 0);
    else
        clip_sample_kernel<float><<<grid, THREADS, 0, s>>>(items, out_h, out_w, (float*)out, sb, sc, st, nrm, reverse ? 1 : 0);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
