// clip_color.hip -- the AVA clip front end (ava_dataset.py:255-365, transform.py:297-517 of the reference): the sampler of
// clip_sample.hip with a colour stage between /255 and the mean/std normalisation -- brightness, contrast and saturation
// in a drawn order, then the PCA lighting shift.  Contrast blends every frame towards ITS OWN mean grey, taken on the frame
// as it stands when contrast runs (resampled, cropped, jittered by the ops drawn before it), so no output pixel can be
// written before a reduction over the whole output window has finished: two kernels.
//
//   clip_gray_mean_kernel    same grid and work split as the sampler.  A thread resamples its RUN = 8 pixels, applies the ops
//       that precede contrast, forms the grey of each and adds them in x order; wave_sum (xor butterfly over 64 lanes), the
//       four wave sums through LDS in wave order, and thread 0 holds the block's partial.  One block per frame: it divides
//       and writes frame_mean.  More: thread 0 stores the partial write-through (agent scope) into the workspace, waits
//       for the store, and takes a ticket from the frame's counter with an agent-scope integer add; the block that draws the
//       last ticket acquires, adds the partials in block order and writes frame_mean.  The order of every addition is fixed
//       by indices, never by arrival, and no floating-point atomic is used: two calls give the same bits.  Blocks of a clip
//       without contrast return at once; the first of each frame writes 0.
//   clip_sample_color_kernel    clip_sample_kernel's work split (8 output x of one row per thread, all three channels,
//       16-byte stores where the address allows, block-uniform descriptor); after the bilinear value: /255, the ops of the
//       clip's record (grey from the thread's own three channel registers, m_t from frame_mean[b, t]), + shift, mean/std by
//       source channel, the optional reversal, the cast.
//
// The tap arithmetic is restated from clip_sample.hip expression by expression (tests/test_gpu_ava_clip.py holds the two
// together through the zero-op record); clip_sample.hip itself is untouched.
#include "focus_common.h"

namespace {

constexpr int RUN = 8;
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / 64;

struct ColorNorm { float a[3], b[3], gw[3]; };      // out = x * a[c'] + b[c'],  a = 1 / std,  b = -mean / std;  grey weights
struct Px { float c0, c1, c2; };                    // one pixel by source channel
struct Ops { int n, k0, k1, k2; float a0, a1, a2; };  // a clip's record in scalars: an indexed copy of it would live in scratch

// The sampler's row set-up (clip_sample.hip): what one output row shares.  ok = false for a descriptor whose rectangle or
// virtual size is empty (the sampler skips it).
struct Row { const uint8_t *row0, *row1; float ly, scale_x; int sw, ox0, flip; bool ok; };
__device__ __forceinline__ Row row_of(const focus_clip_item& it, int t, int y) {
    Row r;
    // memory safety only (the caller validates the rectangle): never read outside [0,H) x [0,W)
    const int sy0 = min(max(it.sy0, 0), it.H - 1), sx0 = min(max(it.sx0, 0), it.W - 1);
    const int sh = min(it.sh, it.H - sy0), sw = min(it.sw, it.W - sx0);
    r.ok = !(it.H <= 0 || it.W <= 0 || sh <= 0 || sw <= 0 || it.rh <= 0 || it.rw <= 0);
    const float scale_y = (float)sh / (float)it.rh;
    r.scale_x = (float)sw / (float)it.rw;
    const float sy = fmaxf(((float)(y + it.oy0) + 0.5f) * scale_y - 0.5f, 0.0f);
    const int y0 = min((int)sy, sh - 1), y1 = min(y0 + 1, sh - 1);
    r.ly = sy - (float)y0;
    const uint8_t* frame = it.src + (int64_t)t * it.frame_stride + (int64_t)sx0 * 3;
    r.row0 = frame + (int64_t)(sy0 + y0) * it.row_stride;
    r.row1 = frame + (int64_t)(sy0 + y1) * it.row_stride;
    r.sw = sw; r.ox0 = it.ox0; r.flip = it.flip;
    return r;
}

// The sampler's taps for output column x, then /255: the pixel in [0,1] by source channel.
__device__ __forceinline__ Px sample_px(const Row& r, int x, int out_w) {
    const int xo = r.flip ? out_w - 1 - x : x;
    const float sx = fmaxf(((float)(xo + r.ox0) + 0.5f) * r.scale_x - 0.5f, 0.0f);
    const int x0 = min((int)sx, r.sw - 1), x1 = min(x0 + 1, r.sw - 1);
    const float lx = sx - (float)x0;
    const uint8_t *p00 = r.row0 + x0 * 3, *p01 = r.row0 + x1 * 3, *p10 = r.row1 + x0 * 3, *p11 = r.row1 + x1 * 3;
    float v[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (float)p00[c] + lx * ((float)p01[c] - (float)p00[c]);      // byte differences are exact
        const float bot = (float)p10[c] + lx * ((float)p11[c] - (float)p10[c]);
        v[c] = (top + r.ly * (bot - top)) * (1.0f / 255.0f);
    }
    return {v[0], v[1], v[2]};
}

__device__ __forceinline__ float gray_of(const ColorNorm& nrm, Px p) {
    return fmaf(nrm.gw[2], p.c2, fmaf(nrm.gw[1], p.c1, nrm.gw[0] * p.c0));
}

// One op on one pixel.  kind is block-uniform; m is the frame's mean grey (contrast only).
__device__ __forceinline__ Px apply_op(int kind, float alpha, float m, const ColorNorm& nrm, Px p) {
    if (kind == FOCUS_COLOR_BRIGHTNESS) return {p.c0 * alpha, p.c1 * alpha, p.c2 * alpha};
    const float other = (kind == FOCUS_COLOR_CONTRAST ? m : gray_of(nrm, p)) * (1.0f - alpha);
    return {fmaf(p.c0, alpha, other), fmaf(p.c1, alpha, other), fmaf(p.c2, alpha, other)};
}
// The first `upto` ops of the record, in its order.
__device__ __forceinline__ Px apply_ops(const Ops& o, int upto, float m, const ColorNorm& nrm, Px p) {
    if (upto > 0) p = apply_op(o.k0, o.a0, m, nrm, p);
    if (upto > 1) p = apply_op(o.k1, o.a1, m, nrm, p);
    if (upto > 2) p = apply_op(o.k2, o.a2, m, nrm, p);
    return p;
}
__device__ __forceinline__ Ops ops_of(const focus_clip_color* col) {
    return {min(max(col->n_ops, 0), 3), col->op[0], col->op[1], col->op[2], col->alpha[0], col->alpha[1], col->alpha[2]};
}
// the position of contrast among the ops, -1 without
__device__ __forceinline__ int contrast_pos(const Ops& o) {
    return (o.n > 0 && o.k0 == FOCUS_COLOR_CONTRAST) ? 0 : (o.n > 1 && o.k1 == FOCUS_COLOR_CONTRAST) ? 1
         : (o.n > 2 && o.k2 == FOCUS_COLOR_CONTRAST) ? 2 : -1;
}

__global__ __launch_bounds__(THREADS) void clip_gray_mean_kernel(const focus_clip_item* __restrict__ items,
                                                                 const focus_clip_color* __restrict__ colors, int out_h, int out_w,
                                                                 float* __restrict__ frame_mean, unsigned* counters, float* partials,
                                                                 ColorNorm nrm) {
    __shared__ float red[WAVES];
    const int t = blockIdx.y, b = blockIdx.z, T = gridDim.y, nblk = gridDim.x;
    const int f = b * T + t;
    const Ops ops = ops_of(colors + b);
    const int pos = contrast_pos(ops);                         // block-uniform; ops [0, pos) run before the grey is taken
    if (pos < 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) frame_mean[f] = 0.0f;
        return;
    }
    const focus_clip_item it = items[b];
    const int runs = (out_w + RUN - 1) / RUN;
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    float sum = 0.0f;
    if (idx < runs * out_h) {
        const int y = idx / runs, xb = (idx - y * runs) * RUN;
        const Row r = row_of(it, t, y);
        const int n = r.ok ? min(RUN, out_w - xb) : 0;         // an empty descriptor: mean 0
#pragma unroll
        for (int j = 0; j < RUN; ++j)
            if (j < n) sum += gray_of(nrm, apply_ops(ops, pos, 0.0f, nrm, sample_px(r, xb + j, out_w)));
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x != 0) return;
    float total = red[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) total += red[w];
    const float count = (float)out_h * (float)out_w;
    if (nblk == 1) {
        frame_mean[f] = total / count;
        return;
    }
    // This lane is the only one of its block that stores or signals.  The partial goes out write-through at agent scope, the
    // wait drains it, then the ticket: the block whose add returns nblk - 1 knows every other partial has left its XCD.
    float* part = partials + (int64_t)f * nblk;
    __hip_atomic_store(part + blockIdx.x, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned ticket = __hip_atomic_fetch_add(counters + f, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != (unsigned)(nblk - 1)) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    float s = 0.0f;
    for (int i = 0; i < nblk; ++i) s += __hip_atomic_load(part + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    frame_mean[f] = s / count;
}

template <typename T>
__global__ __launch_bounds__(THREADS) void clip_sample_color_kernel(const focus_clip_item* __restrict__ items,
                                                                    const focus_clip_color* __restrict__ colors,
                                                                    const float* __restrict__ frame_mean, int out_h, int out_w,
                                                                    T* __restrict__ out, int64_t sb, int64_t sc, int64_t sf,
                                                                    ColorNorm nrm, int reverse) {
    const int runs = (out_w + RUN - 1) / RUN;
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= runs * out_h) return;
    const int y = idx / runs, xb = (idx - y * runs) * RUN;
    const int t = blockIdx.y, b = blockIdx.z;
    const focus_clip_item it = items[b];
    const Ops ops = ops_of(colors + b);
    const float s0 = colors[b].shift[0], s1 = colors[b].shift[1], s2 = colors[b].shift[2];
    const Row r = row_of(it, t, y);
    if (!r.ok) return;
    const float m = contrast_pos(ops) >= 0 ? frame_mean[(int64_t)b * gridDim.y + t] : 0.0f;      // unread without contrast
    // mean/std by SOURCE channel; output channel c shows source channel reverse ? 2 - c : c (selects, no dynamic index)
    const int n = min(RUN, out_w - xb);
    float o0[RUN], o1[RUN], o2[RUN];
#pragma unroll
    for (int j = 0; j < RUN; ++j) {
        if (j < n) {
            const Px p = apply_ops(ops, ops.n, m, nrm, sample_px(r, xb + j, out_w));
            const float q0 = fmaf(p.c0 + s0, nrm.a[0], nrm.b[0]), q1 = fmaf(p.c1 + s1, nrm.a[1], nrm.b[1]),
                        q2 = fmaf(p.c2 + s2, nrm.a[2], nrm.b[2]);
            o0[j] = reverse ? q2 : q0; o1[j] = q1; o2[j] = reverse ? q0 : q2;
        } else {
            o0[j] = o1[j] = o2[j] = 0.0f;
        }
    }
    T* p0 = out + (int64_t)b * sb + (int64_t)t * sf + (int64_t)y * out_w + xb;
    T *p1 = p0 + sc, *p2 = p1 + sc;
    const bool full = n == RUN;
    if (full && (reinterpret_cast<uintptr_t>(p0) & 15) == 0) st8<T>(p0, o0);
    else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) if (j < n) st<T>(p0 + j, o0[j]);
    }
    if (full && (reinterpret_cast<uintptr_t>(p1) & 15) == 0) st8<T>(p1, o1);
    else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) if (j < n) st<T>(p1 + j, o1[j]);
    }
    if (full && (reinterpret_cast<uintptr_t>(p2) & 15) == 0) st8<T>(p2, o2);
    else {
#pragma unroll
        for (int j = 0; j < RUN; ++j) if (j < n) st<T>(p2 + j, o2[j]);
    }
}

// grid x of both kernels, or -1 for a window the index arithmetic cannot hold
int64_t blocks_per_frame(int out_h, int out_w) {
    const int64_t work = (int64_t)((out_w + RUN - 1) / RUN) * out_h;
    if (work > (int64_t)0x7fffffff - THREADS) return -1;
    return cdiv64(work, THREADS);
}

}  // namespace

extern "C" size_t focus_clip_color_workspace_bytes(int n_clips, int T, int out_h, int out_w) {
    if (n_clips <= 0 || T <= 0 || out_h <= 0 || out_w <= 0) return 0;
    const int64_t nblk = blocks_per_frame(out_h, out_w);
    if (nblk < 0) return 0;
    return (size_t)n_clips * (size_t)T * (size_t)(1 + nblk) * 4;       // one counter and nblk partials per frame
}

extern "C" int focus_clip_gray_mean(const focus_clip_item* items, const focus_clip_color* colors, int n_clips, int T, int out_h,
                                    int out_w, const float* gray_w, float* frame_mean, void* workspace, size_t workspace_bytes,
                                    void* stream) {
    if (!items || !colors || !gray_w || !frame_mean || !workspace) return FOCUS_ERR_NULL;
    if (n_clips <= 0 || T <= 0) return FOCUS_OK;
    if (out_h <= 0 || out_w <= 0 || T > 65535 || n_clips > 65535) return FOCUS_ERR_SHAPE;
    const int64_t nblk = blocks_per_frame(out_h, out_w);
    if (nblk < 0) return FOCUS_ERR_SHAPE;
    if (!focus_aligned(workspace, 4) || !focus_aligned(frame_mean, 4)) return FOCUS_ERR_ALIGN;
    if (workspace_bytes < focus_clip_color_workspace_bytes(n_clips, T, out_h, out_w)) return FOCUS_ERR_WORKSPACE;
    ColorNorm nrm = {};
    for (int c = 0; c < 3; ++c) nrm.gw[c] = gray_w[c];
    hipStream_t s = (hipStream_t)stream;
    unsigned* counters = (unsigned*)workspace;
    float* partials = (float*)workspace + (size_t)n_clips * T;
    if (nblk > 1 && hipMemsetAsync(counters, 0, (size_t)n_clips * T * 4, s) != hipSuccess) return FOCUS_ERR_LAUNCH;
    const dim3 grid((unsigned)nblk, (unsigned)T, (unsigned)n_clips);
    clip_gray_mean_kernel<<<grid, THREADS, 0, s>>>(items, colors, out_h, out_w, frame_mean, counters, partials, nrm);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}

extern "C" int focus_clip_sample_color(const focus_clip_item* items, const focus_clip_color* colors, const float* frame_mean,
                                       int n_clips, int T, int out_h, int out_w, void* out, int64_t sb, int64_t sc, int64_t st,
                                       const float* mean, const float* std, const float* gray_w, int reverse, int dtype,
                                       void* stream) {
    if (!items || !colors || !frame_mean || !out || !mean || !std || !gray_w) return FOCUS_ERR_NULL;
    if (n_clips <= 0 || T <= 0) return FOCUS_OK;
    if (out_h <= 0 || out_w <= 0 || T > 65535 || n_clips > 65535) return FOCUS_ERR_SHAPE;
    const int64_t nblk = blocks_per_frame(out_h, out_w);
    if (nblk < 0) return FOCUS_ERR_SHAPE;
    if (dtype != FOCUS_F32 && dtype != FOCUS_BF16) return FOCUS_ERR_DTYPE;
    ColorNorm nrm;
    for (int c = 0; c < 3; ++c) {
        nrm.a[c] = (float)(1.0 / (double)std[c]);
        nrm.b[c] = (float)(-(double)mean[c] / (double)std[c]);
        nrm.gw[c] = gray_w[c];
    }
    const dim3 grid((unsigned)nblk, (unsigned)T, (unsigned)n_clips);
    hipStream_t s = (hipStream_t)stream;
    if (dtype == FOCUS_BF16)
        clip_sample_color_kernel<bf16_t><<<grid, THREADS, 0, s>>>(items, colors, frame_mean, out_h, out_w, (bf16_t*)out, sb, sc, st,
                                                                  nrm, reverse ? 1 : 0);
    else
        clip_sample_color_kernel<float><<<grid, THREADS, 0, s>>>(items, colors, frame_mean, out_h, out_w, (float*)out, sb, sc, st,
                                                                 nrm, reverse ? 1 : 0);
    FOCUS_CHECK_LAUNCH();
    return FOCUS_OK;
}
